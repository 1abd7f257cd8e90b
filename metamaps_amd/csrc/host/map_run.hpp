// One run of mapDirectly / index / mapAgainstIndex (MapRun), and what only it uses: the formatter of the mapping lines.
#pragma once
#include "../cpu_budget.hpp"
#include "../task_pool.hpp"
#include "classify_run.hpp"
#include "cli_device.hpp"
#include "cli_switches.hpp"
#include "edit_dist.hpp"
#include "paf_out.hpp"
#include "bam_out.hpp"
#include "fast_format.hpp"
#include "id_set.hpp"
#include "query_reader.hpp"
#include <climits>
#include <cmath>
#include <fstream>
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

// records of one batch -> the text of PREFIX (computeMap.hpp:565-581 + the two fields of mapWrap.h:311-320), reads in order
// fields 10 and 13 of a mapping line are functions of (conserved sketches, sketch size) alone: formatted once per pair and kept.  The table belongs
// to the CALLER (one per formatting slot of a worker thread) and lives as long as that thread: the pool threads of format_records are new with every
// batch, and a table that was theirs (thread_local) was rebuilt — 0.8 MB cleared, every pair formatted again — by every one of them for every batch:
// 19 ms per batch of 85 000 lines, the whole of a worker's "finish" time.
struct FormatCache {
  struct Pair { uint64_t key; char ids[16], corr[16]; uint8_t n_ids, n_corr; double ident; };   // ident: the printed identity read back / 100 (what classify parses, fEM.h:264)
  static constexpr size_t CB = 1 << 14;
  std::vector<Pair> slots; int k = -1;
  void prepare(int k_now) { if (slots.size() != CB || k != k_now) { slots.assign(CB, Pair{~0ull, {0}, {0}, 0, 0, 0.0}); k = k_now; } }
};
static void format_range(const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off,
                         const std::vector<mm_map_record>& rec, const std::vector<std::string>& cname, const std::vector<int>& clen, int k, size_t r0, size_t r1, std::string& out,
                         FormatCache& fc, std::vector<LineMeta>* meta, const int64_t* raw_end /* --hpc: field 9 of every record; else nullptr */) {
  out.clear();
  if (meta) { meta->clear(); meta->reserve((size_t)(off[r1] - off[r0])); }
  out.reserve((size_t)(off[r1] - off[r0]) * 160);
  // no printf anywhere on the line (fast_format.hpp) — 4.2 M lines took 2 s of the mapping phase of a million reads
  using Pair = FormatCache::Pair;
  fc.prepare(k);
  std::vector<Pair>& cache = fc.slots;
  std::string tmp;
  for (size_t r = r0; r < r1; ++r) {
    const int len = lens[r];
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      const mm_map_record& x = rec[(size_t)i];
      const uint64_t key = (uint64_t)(uint32_t)x.sketch << 32 | (uint32_t)x.shared;
      Pair& P = cache[(size_t)((key * 0x9E3779B97F4A7C15ull) >> 50)];
      if (P.key != key) {
        float id; mm_identity(x.shared, x.sketch, k, &id, nullptr);
        tmp.clear(); append_g6(tmp, (double)id);                   // operator<<(float): %g with 6 significant digits; printed, then re-parsed (mapWrap.h:237)
        P.n_ids = (uint8_t)tmp.size(); memcpy(P.ids, tmp.data(), tmp.size());
        const double reported = strtod(tmp.c_str(), nullptr) / 100.0;
        P.ident = reported;
        const float corrected = std::exp(-(1 - reported));        // mapWrap.h:311
        tmp.clear(); append_g6(tmp, (double)(corrected * 100));
        P.n_corr = (uint8_t)tmp.size(); memcpy(P.corr, tmp.data(), tmp.size());
        P.key = key;
      }
      const size_t line_beg = out.size();
      out += names[r];
      out += ' '; append_int(out, len); out += " 0 "; append_int(out, len - 1); out += ' '; out += x.strand == 1 ? '+' : '-'; out += ' ';
      out += cname[(size_t)x.ref_contig];
      out += ' '; append_int(out, clen[(size_t)x.ref_contig]);
      out += ' '; append_int(out, x.ref_start); out += ' '; append_int(out, raw_end ? (long long)raw_end[(size_t)i] : (long long)x.ref_start + len - 1);
      out += ' '; out.append(P.ids, P.n_ids);
      out += ' '; append_int(out, x.shared); out += ' '; append_int(out, x.sketch);
      out += ' '; out.append(P.corr, P.n_corr);
      const size_t ls = out.size();
      out += ' '; append_g6(out, x.mapq);                          // :318-320
      if (meta) meta->push_back(LineMeta{(uint32_t)line_beg, (uint32_t)(ls - line_beg), (uint32_t)(out.size() - line_beg), (int32_t)x.ref_contig, (int32_t)len, (int32_t)x.ref_start, (int32_t)(raw_end ? raw_end[(size_t)i] : (int64_t)x.ref_start + len - 1),
                                         P.ident, mapq_as_classify_reads_it(out.data() + ls + 1, out.size() - ls - 1)});
      out += '\n';
    }
  }
}
// the mapping lines of a batch (mapWrap.h:300-323): ranges of reads formatted by a few threads, joined in read order
void format_records(const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off,
                    const std::vector<mm_map_record>& rec, const std::vector<std::string>& cname, const std::vector<int>& clen, int k, std::string& out, std::vector<LineMeta>* meta,
                    const int64_t* raw_end, const CliSwitches& sw) {
  const size_t n = names.size();
  const size_t per_part = sw.format_part;
  const size_t T = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)std::max(per_part < 10000 ? 8u : 1u, mm::cpu_budget() / 4), rec.size() / per_part + 1}));   // (a quarter of the CPU budget per worker: four workers rarely format at the same moment)
  static thread_local std::vector<FormatCache> caches(8);          // (the calling thread's: a worker of mapDirectly formats batch after batch)
  if (T == 1) { format_range(names, lens, off, rec, cname, clen, k, 0, n, out, caches[0], meta, raw_end); return; }
  std::vector<size_t> cut(T + 1, n);
  cut[0] = 0;
  { size_t t = 1; for (size_t r = 0; r < n && t < T; ++r) if ((uint64_t)off[r] >= (uint64_t)rec.size() * t / T) cut[t++] = r; }
  static thread_local std::vector<std::string> part_store(8);      // (kept with their capacity: fresh text buffers are page faults, batch after batch)
  std::vector<std::string>& part = part_store;
  FormatCache* const fcs = caches.data();
  static thread_local std::vector<std::vector<LineMeta>> meta_store(8);
  std::vector<std::vector<LineMeta>>& metas = meta_store;        // (the CALLING thread's: the helpers below must not name the thread_local themselves)
  const auto q0 = std::chrono::steady_clock::now();
  std::vector<double> took(T, 0.0);
  auto timed = [&](size_t t) { const auto a = std::chrono::steady_clock::now(); format_range(names, lens, off, rec, cname, clen, k, cut[t], cut[t + 1], part[t], fcs[t], meta ? &metas[t] : nullptr, raw_end);
                               took[t] = std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
  static thread_local TaskPool helpers(7);                         // (task_pool.hpp: the calling worker's own helpers, there from batch to batch)
  const auto q1 = q0;
  helpers.run(T, timed);
  const auto q2 = std::chrono::steady_clock::now();
  size_t total = 0; for (size_t t = 0; t < T; ++t) total += part[t].size();
  out.clear(); out.reserve(total);
  if (meta) { meta->clear(); meta->reserve(rec.size()); }
  for (size_t t = 0; t < T; ++t) {
    if (meta) for (LineMeta lm : metas[t]) { lm.beg += (uint32_t)out.size(); meta->push_back(lm); }
    out += part[t];
  }
  if (sw.format_trace) {
    const auto q3 = std::chrono::steady_clock::now();
    double mx = 0; for (double x : took) mx = std::max(mx, x);
    fprintf(stderr, "FORMAT_TRACE %zu records, %zu threads: all parts %.2f ms (own part %.2f ms, slowest part %.2f ms), join text %.2f ms\n", rec.size(), T,
            std::chrono::duration<double, std::milli>(q2 - q1).count(), took[0] * 1e3, mx * 1e3, std::chrono::duration<double, std::milli>(q3 - q2).count());
  }
}

// One run of mapDirectly / index / mapAgainstIndex.  The state every stage shares lives in the object; the stages are its methods, in the order run()
// calls them: parameters -> devices -> reference (parsed, packed, uploaded) or stored index -> chunk plan -> placement of the chunk indexes
// (replicated / sharded / streamed) -> read batches through the worker pipeline (replicated) or chunk-major rounds with the exchange of the
// records (sharded / streamed) -> writers -> optionally classify in-process.  (Until round 5 this was one 800-line function.)
struct MapRun {
  const Options& o; const CliSwitches& sw; const std::string mode;
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
  const bool edit = o.v.count("edit-distance") != 0;             // --edit-distance: the packed reference stays on every device, a batch's reads live until its distances are fetched (edit_dist.hpp)
  const bool paf = o.v.count("paf") != 0;                        // --paf (implies --edit-distance): the same call also gives the CIGARs of PREFIX.paf (paf_out.hpp)
  const bool bam = o.v.count("bam") != 0;                        // --bam (implies --edit-distance): that alignment also becomes the records of PREFIX.bam, encoded and deflated on the device (bam_out.hpp)
  std::string bam_head;                                          // the header of every PREFIX.bam as BGZF members (the contigs are the run's)
  std::vector<int> clen_raw; std::vector<mm_hpc_map*> hpc_map;
  struct Chunk { int first, count; std::string file; };
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
  // what a worker hands to the writer: the finished text of one batch
  struct Done { size_t file = 0; std::vector<std::string> names; std::vector<int> lens; std::vector<int> clens /* --hpc: the compressed lengths (lens stay raw) */; std::vector<int64_t> off; std::string text; std::string gz /* --compress-output: the text as BGZF members */; std::string edit /* --edit-distance: the batch's lines of PREFIX.editDistances */; std::string paf /* --paf: the batch's lines of PREFIX.paf */; std::string bam /* --bam: the batch's records of PREFIX.bam as BGZF members */; std::vector<LineMeta> meta; double t_mapq = 0, t_fetch = 0, t_format = 0; };
  // --then-classify: the batches of every query file as they were written, in order (text + the parsed fields of every line): what classify takes instead of the file
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

  MapRun(const Options& o_, const std::string& mode_, const CliSwitches& sw_) : o(o_), sw(sw_), mode(mode_), from_index(mode_ == "mapAgainstIndex"), only_index(mode_ == "index") {}
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
      std::ifstream a(ipre + ".arguments");
      if (!a.is_open()) die("Cannot open file " + ipre + ".arguments for deserialization.");
      std::string key, val; std::map<std::string, std::string> kv;
      while (a >> key && std::getline(a, val)) { while (!val.empty() && val[0] == ' ') val.erase(0, 1); kv[key] = val; }
      for (const char* need : {"kmerSize", "windowSize", "minReadLength", "percentageIdentity", "p_value", "referenceSize", "maximumMemory", "reference"})
        if (!kv.count(need)) die("Index " + ipre + " is incomplete (" + need + " missing in .arguments)");
      k = std::stoi(kv["kmerSize"]); w = std::stoi(kv["windowSize"]); minLen = std::stoi(kv["minReadLength"]); pi = std::stof(kv["percentageIdentity"]);
      pval = std::stod(kv["p_value"]); refSize = std::stoull(kv["referenceSize"]); maxMem = std::stoull(kv["maximumMemory"]); ref = kv["reference"];
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
    reader.th = std::thread([this]() { QueryReader(reader, queries, BATCH_READS, BATCH_BASES, devs[0].phys, pc, mapped, sw).run(); }); }
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
    struct Group { std::deque<std::string> seq; std::vector<std::string> names; uint64_t bases = 0; };
    const uint64_t GROUP_BASES = sw.ref_group_bases;
    std::vector<std::vector<mm_seqset*>> parts(only_index ? 1 : G);
    double t_pack = 0;
    auto consume = [&](Group& g) {                               // names and lengths in file order, then pack + upload to every device
      for (size_t i = 0; i < g.seq.size(); ++i) { cname.push_back(std::move(g.names[i])); clen.push_back((int)g.seq[i].size()); ref_bases += g.seq[i].size(); }
      const auto t0 = std::chrono::steady_clock::now();
      on_each(parts.size(), [&](size_t d) {
        mm_seqset* p; ck(devs[d].ctx, mm_seqset_create(devs[d].ctx, &p), "seqset");
        for (auto& q : g.seq) ck(devs[d].ctx, mm_seqset_add_view(p, q.data(), (int64_t)q.size()), "add contig");
        ck(devs[d].ctx, mm_seqset_upload(p), "upload reference");
        parts[d].push_back(p);
      });
      t_pack += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    // records of `f` (all, or those that start before `stop` in memory mode) in groups of GROUP_BASES handed to `emit`; false when the
    // reader gave up before `stop` (a truncated quality string ends the file for kseq, kseq.h:204)
    auto parse_groups = [&](SeqFile& f, size_t stop, const std::function<void(std::unique_ptr<Group>)>& emit) -> bool {
      auto g = std::make_unique<Group>();
      bool ok = true;
      for (;;) {
        if (stop != (size_t)-1) { const size_t ps = f.peek_start(); if (ps == (size_t)-1 || ps >= stop) break; }
        if (!f.next()) { ok = stop == (size_t)-1; break; }
        g->names.push_back(f.name);
        if (f.view) g->seq.emplace_back(f.view, f.view_len); else { g->seq.push_back(std::move(f.seq)); f.seq.clear(); }
        g->bases += g->seq.back().size();
        if (g->bases >= GROUP_BASES) { emit(std::move(g)); g = std::make_unique<Group>(); }
      }
      if (!g->seq.empty()) emit(std::move(g));
      return ok;
    };
    MappedFile rmf;
    if (!sw.no_mmap && !sw.ref_sequential && rmf.open(ref)) {
      // A plain file: blocks of the mapping parsed by several threads (the block parser of the query files below: a block's records
      // count only once the block before it has been seen to end exactly where this one starts), consumed — packed, uploaded — in file
      // order.  The winSketch.hpp:242-252 loop reads contig by contig; here the text of at most P + 2 blocks of 256 MB is resident, and the
      // mapped pages of a block are given back once it is consumed (they would count as resident until the end otherwise: 27 GB).
      const size_t blk = sw.ref_block_bytes;
      const size_t nb = std::max<size_t>(1, (rmf.size + blk - 1) / blk);
      std::vector<size_t> start(nb + 1, rmf.size);
      start[0] = 0;
      struct Block { std::vector<std::unique_ptr<Group>> out; size_t next = 0; bool done = false, empty = false, over = false; };
      std::vector<Block> blocks(nb);
      std::mutex bm; std::condition_variable bcv; size_t next_block = 0, consumed = 0; bool abandon = false;
      const unsigned P = (unsigned)std::max<size_t>(1, std::min<size_t>({nb, (size_t)8, (size_t)std::max(1u, mm::cpu_budget() / 2)}));
      auto worker = [&]() {
        for (;;) {
          size_t j;
          {
            std::unique_lock<std::mutex> lk(bm);
            bcv.wait(lk, [&] { return abandon || next_block >= nb || next_block < consumed + P + 1; });   // not too far ahead of the consumer
            if (abandon || next_block >= nb) return;
            j = next_block++;
          }
          if (j > 0) start[j] = rmf.sync(j * blk, std::min(rmf.size, (j + 1) * blk));
          Block& B = blocks[j];
          const size_t lim = std::min(rmf.size, (j + 1) * blk);
          if (j == 0 || start[j] < lim) {
            SeqFile f(rmf.data, j == 0 ? 0 : start[j], rmf.size);
            B.over = !parse_groups(f, lim, [&](std::unique_ptr<Group> g) { B.out.push_back(std::move(g)); });
            B.next = f.peek_start();
          } else B.empty = true;
          { std::lock_guard<std::mutex> lk(bm); B.done = true; }
          bcv.notify_all();
        }
      };
      std::vector<std::thread> pool;
      for (unsigned t = 0; t < P; ++t) pool.emplace_back(worker);
      size_t expect = 0; bool chain_ok = true, file_over = false;
      for (size_t j = 0; j < nb && chain_ok && !file_over; ++j) {
        { std::unique_lock<std::mutex> lk(bm); bcv.wait(lk, [&] { return blocks[j].done; }); }
        Block& B = blocks[j];
        if (!B.empty) {
          if (j > 0 && start[j] != expect) { chain_ok = false; break; }
          for (auto& g : B.out) consume(*g);
          B.out.clear();
          if (B.over || B.next == (size_t)-1) { file_over = true; break; }
          expect = B.next;
        } else if (expect < std::min(rmf.size, (j + 1) * blk)) { chain_ok = false; break; }
        { std::lock_guard<std::mutex> lk(bm); consumed = j + 1; } bcv.notify_all();
        if (j > 0) rmf.drop(((j - 1) * blk) & ~(size_t)4095, (j * blk) & ~(size_t)4095);   // (block j - 1: its last record may end inside block j, parsed by now)
      }
      { std::lock_guard<std::mutex> lk(bm); abandon = true; } bcv.notify_all();
      for (auto& t : pool) t.join();
      if (!chain_ok) {                                           // a block did not start where the parse stood: the rest sequentially, from there
        for (auto& B : blocks) B.out.clear();
        SeqFile f(rmf.data, expect, rmf.size);
        parse_groups(f, (size_t)-1, [&](std::unique_ptr<Group> g) { consume(*g); });
      }
    } else {
      // gzip, pipes: a parser thread fills groups, the main thread packs and uploads each while the next one is parsed.  Host memory: two groups.
      std::mutex gm; std::condition_variable gcv; std::deque<std::unique_ptr<Group>> ready; bool parsed = false;
      double t_gzip = -1;                                        // the device gzip reader's wall time (its phase line), -1 if zlib read the file
      std::thread parser([&]() {
        if (!sw.gzip_host_inflate && is_plain_gzip_file(ref)) {   // plain gzip: inflated on the device, on a context of the parser's own
          const auto g_t0 = std::chrono::steady_clock::now();
          mm_ctx* gctx = nullptr;
          if (mm_ctx_create(devs[0].phys, &gctx) != MM_OK) die("cannot create the reference reader's inflate context");
          {
            DeviceGzip z(gctx, ref);
            SeqFile f([&](std::vector<unsigned char>& buf) -> size_t { return z.fill(buf); });
            parse_groups(f, (size_t)-1, [&](std::unique_ptr<Group> g) {
              std::unique_lock<std::mutex> lk(gm); gcv.wait(lk, [&] { return ready.size() < 2; }); ready.push_back(std::move(g)); gcv.notify_all();
            });
          }
          mm_ctx_destroy(gctx);
          std::lock_guard<std::mutex> lk(gm); parsed = true; gcv.notify_all();
          t_gzip = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
          return;
        }
        SeqFile f(ref);
        parse_groups(f, (size_t)-1, [&](std::unique_ptr<Group> g) {
          std::unique_lock<std::mutex> lk(gm); gcv.wait(lk, [&] { return ready.size() < 2; }); ready.push_back(std::move(g)); gcv.notify_all();
        });
        std::lock_guard<std::mutex> lk(gm); parsed = true; gcv.notify_all();
      });
      for (;;) {
        std::unique_ptr<Group> g;
        { std::unique_lock<std::mutex> lk(gm); gcv.wait(lk, [&] { return !ready.empty() || parsed; }); if (ready.empty()) break; g = std::move(ready.front()); ready.pop_front(); gcv.notify_all(); }
        consume(*g);
      }
      parser.join();
      if (t_gzip >= 0) pc.add("1g reference gzip reader (device inflate + parse, inside 1)", t_gzip);
    }
    on_each(parts.size(), [&](size_t d) {
      if (parts[d].size() == 1) { refset[d] = parts[d][0]; return; }
      if (parts[d].empty()) { ck(devs[d].ctx, mm_seqset_create(devs[d].ctx, &refset[d]), "seqset"); ck(devs[d].ctx, mm_seqset_upload(refset[d]), "upload reference"); return; }
      ck(devs[d].ctx, mm_seqset_concat(devs[d].ctx, parts[d].data(), (int)parts[d].size(), &refset[d]), "reference");
      for (auto* p : parts[d]) mm_seqset_destroy(p);
    });
    pc.lap("1 reference parse + pack + upload");
    pc.add("2 reference pack+upload (inside 1)", t_pack);
    if (hpc) compress_reference();
    if (!only_index) { if (!sw.late_reader) start_reader(); start_prewarm(); }   // (MM_CLI_LATE_READER: measurement aid — the reader starts when the index is built)
    query_free();                                                // the packed reference now lives on the device (0.25 B per base, for as long as chunks are cut out of it): what is left is what the indexes get
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
    { std::ofstream flag(ipre + ".index"); if (!flag.is_open()) die("Cannot open " + ipre + ".index"); flag << 0 << "\n"; }   // mapWrap.h:363-366
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
    std::ofstream args(ipre + ".arguments");
    if (!args.is_open()) die("Cannot open file " + ipre + ".arguments for serialization.");
    args.precision(17);
    args << "kmerSize " << k << "\nwindowSize " << w << "\nminReadLength " << minLen << "\npercentageIdentity " << pi << "\np_value " << pval
         << "\nreferenceSize " << refSize << "\nmaximumMemory " << maxMem << "\nreference " << ref << "\n";
    std::ofstream cf(ipre + ".contigs");
    for (size_t c = 0; c < chunks.size(); ++c)
      for (int i = chunks[c].first; i < chunks[c].first + chunks[c].count; ++i) cf << cname[(size_t)i] << "\t" << clen[(size_t)i] << "\t" << c + 1 << "\n";
    std::ofstream flag(ipre + ".index");                       // mapWrap.h:395-402
    flag << 1 << "\n";
    for (auto& fn : chunk_files) { flag << fn << "\n"; std::cout << "Stored state in file " << fn << "\n"; }
    mm_ctx_destroy(ctx0);
    return 0;
  }

  // `metamaps mapAgainstIndex`: the chunk list and the contig table of a stored index (mapWrap.h:443-554)
  void read_index_files() {
    std::ifstream flag(ipre + ".index");
    if (!flag.is_open()) die("Index " + ipre + " not found (" + ipre + ".index)");
    int done = 0; flag >> done;
    if (done != 1) die("Index " + ipre + " is not complete.");    // mapWrap.h:466-470
    std::vector<std::string> chunk_files; std::string fn;
    while (flag >> fn) chunk_files.push_back(fn);
    std::ifstream cf(ipre + ".contigs");
    if (!cf.is_open()) die("Cannot open " + ipre + ".contigs");
    std::vector<int> chunk_of; std::string line;
    while (std::getline(cf, line)) {
      auto fl = split(line, "\t");
      if (fl.size() != 3) die("Weird line in " + ipre + ".contigs");
      cname.push_back(fl[0]); clen.push_back(std::stoi(fl[1])); chunk_of.push_back(std::stoi(fl[2])); ref_bases += (uint64_t)clen.back();
    }
    for (size_t c = 0; c < chunk_files.size(); ++c) {
      int first = -1, count = 0;
      for (size_t i = 0; i < chunk_of.size(); ++i) if (chunk_of[i] == (int)c + 1) { if (first < 0) first = (int)i; ++count; }
      chunks.push_back(Chunk{first < 0 ? 0 : first, count, chunk_files[c]});
    }
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
    if (edit && place != Place::Replicated) die(std::string(bam ? "--bam" : paf ? "--paf" : "--edit-distance") + " needs the whole reference resident on every device, and this index does not fit one: run without it");
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
      if (!edit) drop_refsets();
      pc.lap("3 index build");
    }
  }

  mm_seqset* upload_batch(mm_ctx* ctx, const Batch& bt) {
    mm_seqset* reads; ck(ctx, mm_seqset_create(ctx, &reads), "seqset");
    if (bt.nt16) for (size_t r = 0; r < bt.names.size(); ++r) ck(ctx, mm_seqset_add_nt16(reads, (const uint8_t*)bt.seq_of(r), (int64_t)bt.lens[r], bt.rev[r]), "add read");
    else for (size_t r = 0; r < bt.names.size(); ++r) ck(ctx, mm_seqset_add_view(reads, bt.seq_of(r), (int64_t)bt.lens[r]), "add read");
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
  std::unique_ptr<Done> finish_mapping(mm_ctx* ctx, size_t dev, mm_mapping* m, std::vector<std::string>&& names, std::vector<int>&& lens, std::vector<int>&& clens, size_t file, mm_seqset* reads = nullptr) {   // mapping qualities + text; consumes m (and the reads that --edit-distance has kept)
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
    BatchAlignment al;                                             // one fetch serves .editDistances, .paf and .bam
    if (reads && (paf || bam)) {
      fetch_alignment(ctx, m, reads, refset[dev], pi, rec.size(), al);
      edit_distance_text(al.dist.data(), al.first.data(), al.last.data(), dn->names, dn->off, rec, cname, dn->edit);
      if (paf) paf_text(al, dn->names, dn->lens, dn->off, rec, cname, clen, dn->paf);
    } else if (reads) edit_distance_lines(ctx, m, reads, refset[dev], pi, dn->names, dn->off, rec, cname, dn->edit);
    if (reads && !bam) { mm_seqset_destroy(reads); reads = nullptr; }
    mm_mapping_destroy(m);
    const auto f2 = std::chrono::steady_clock::now();
    format_records(dn->names, dn->lens, dn->off, rec, cname, hpc ? clen_raw : clen, k, dn->text, keep_lines ? &dn->meta : nullptr, hpc ? raw_end.data() : nullptr, sw);
    if (reads) { bam_members(ctx, reads, refset[dev], al, rec, dn->names, dn->off, dn->text, dn->bam); mm_seqset_destroy(reads); }   // --bam: the mapping qualities come from the formatted lines; the reads have stayed for SEQ
    if (compress) deflate_text(ctx, *dn);
    const auto f3 = std::chrono::steady_clock::now();
    pc.add("7a mapping qualities + offsets", std::chrono::duration<double>(f1 - f0).count());
    pc.add("7b fetch records", std::chrono::duration<double>(f2 - f1).count());
    pc.add("7c format", std::chrono::duration<double>(f3 - f2).count());
    dn->t_mapq = std::chrono::duration<double>(f1 - f0).count(); dn->t_fetch = std::chrono::duration<double>(f2 - f1).count(); dn->t_format = std::chrono::duration<double>(f3 - f2).count();
    return dn;
  }
  // the text of a batch as BGZF members (mm_bgzf_deflate: blocks of 65 280 bytes, each a member of its own, so the batches' members
  // concatenate in output order); the text itself is kept only where --then-classify takes its lines from memory
  void deflate_text(mm_ctx* ctx, Done& dn) {
    const auto z0 = std::chrono::steady_clock::now();
    dn.gz.resize((size_t)mm_bgzf_deflate_bound((int64_t)dn.text.size()));
    int64_t nbytes = 0; int32_t nblocks = 0;
    ck(ctx, mm_bgzf_deflate(ctx, (const uint8_t*)dn.text.data(), (int64_t)dn.text.size(), (uint8_t*)&dn.gz[0], (int64_t)dn.gz.size(), &nbytes, &nblocks), "deflate the mappings");
    dn.gz.resize((size_t)nbytes);
    if (!keep_lines) std::string().swap(dn.text);
    pc.add("7d deflate", std::chrono::duration<double>(std::chrono::steady_clock::now() - z0).count());
  }
  void write_all(const std::function<std::unique_ptr<Done>(size_t, size_t)>& next /* (file, seq): batch `seq` if it belongs to that file, nullptr once the file has ended */) {
    size_t seq = 0;
    for (size_t fi = 0; fi < queries.size(); ++fi) {
      const std::string& prefix = prefixes[fi];
      if (compress) ::unlink(prefix.c_str());                    // (classify prefers a plain PREFIX: one left from an earlier run must not shadow PREFIX.gz)
      const std::string out_name = compress ? prefix + ".gz" : prefix;
      std::ofstream out(out_name, std::ios::binary), unm(prefix + ".meta.unmappedReadsLengths");
      if (!out.is_open()) die("Cannot open output file " + out_name);
      std::ofstream ed; if (edit) { ed.open(prefix + ".editDistances", std::ios::binary); if (!ed.is_open()) die("Cannot open output file " + prefix + ".editDistances"); }
      std::ofstream pf; if (paf) { pf.open(prefix + ".paf", std::ios::binary); if (!pf.is_open()) die("Cannot open output file " + prefix + ".paf"); }
      std::ofstream bf; if (bam) { bf.open(prefix + ".bam", std::ios::binary); if (!bf.is_open()) die("Cannot open output file " + prefix + ".bam"); bf.write(bam_head.data(), (std::streamsize)bam_head.size()); }
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
        if (edit) { ed << d->edit; std::string().swap(d->edit); }
        if (paf) { pf << d->paf; std::string().swap(d->paf); }
        if (bam) { bf.write(d->bam.data(), (std::streamsize)d->bam.size()); std::string().swap(d->bam); }
        std::string().swap(d->gz);
        if (keep_lines) { if (kept.size() <= fi) kept.resize(fi + 1); d->names.clear(); d->names.shrink_to_fit(); kept[fi].push_back(std::move(d)); }
      }
      if (keep_lines && kept.size() <= fi) kept.resize(fi + 1);
      static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0}; if (compress) out.write((const char*)eof, 28);
      out.close();
      if (!out) die("Error writing " + out_name);
      if (bam) { bf.write((const char*)eof, 28); bf.close(); if (!bf) die("Error writing " + prefix + ".bam"); }
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
    // ---- workers: four contexts per device (--workers-per-gpu; three until round 4: with ten batches of 10^5 reads in one file the GPU idled 60 % of the mapping phase), so that packing, result download and text formatting of one batch overlap the
    // kernels of the other; the device's chunk indexes are shared (read-only) by its contexts
    // The kernels of a batch fill the device; batches mapped side by side only take turns on it, and four workers that start together
    // then also finish together: they packed, fetched and formatted at the same time with the device idle, and mapped at the same time
    // in each other's way (the done-times of the workers came in groups of four, 60 ms apart).  So at most MAP_SLOTS batches per device are
    // inside their mapping section at a time (two: one fills the host-side gaps of the other), which staggers the workers.
    const size_t MAP_SLOTS = sw.map_slots;
    struct Slots { std::mutex m; std::condition_variable cv; size_t free_ = 0;
                   void acquire() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return free_ > 0; }); --free_; }
                   void release() { { std::lock_guard<std::mutex> lk(m); ++free_; } cv.notify_one(); } };
    std::vector<Slots> map_slots(G);
    for (auto& sl : map_slots) sl.free_ = MAP_SLOTS;
    std::vector<std::thread> workers;
    for (size_t d = 0; d < G; ++d) for (size_t wi = 0; wi < WPD; ++wi) workers.emplace_back([&, d, wi]() {
      mm_ctx* ctx = wi == 0 ? devs[d].ctx : wctx[d * WPD + wi];
      if (!ctx && mm_ctx_create(devs[d].phys, &ctx) != MM_OK) die("cannot create a worker context");
      while (std::unique_ptr<Batch> bt = reader.take()) {
        const auto t0 = std::chrono::steady_clock::now();
        mm_seqset* reads = upload_batch(ctx, *bt);
        std::vector<int> clens; if (hpc) clens = compressed_lengths(ctx, reads);
        const auto t1 = std::chrono::steady_clock::now();
        std::vector<mm_mapping*> parts;
        map_slots[d].acquire();
        const auto t1a = std::chrono::steady_clock::now();
        for (size_t c = 0; c < NC; ++c) parts.push_back(map_chunk(ctx, devs[d].idx[c], reads, c ? parts[0] : nullptr));
        map_slots[d].release();
        mm_map_stats gst{}; if (sw.timing) mm_mapping_get_stats(parts[0], &gst);   // (device time of the batch's stages by the library's own events)
        mm_mapping* m = parts[0];
        if (parts.size() > 1) {                                   // unifyFiles: read-wise concatenation in chunk order
          ck(ctx, mm_mapping_concat(ctx, parts.data(), chunk_base.data(), (int)parts.size(), &m), "merge chunks");
          for (auto* pm : parts) mm_mapping_destroy(pm);
        }
        if (!edit) { mm_seqset_destroy(reads); reads = nullptr; }
        const auto t2 = std::chrono::steady_clock::now();
        const size_t seq = bt->seq;
        auto dn = finish_mapping(ctx, d, m, std::move(bt->names), std::move(bt->lens), std::move(clens), bt->file, reads);
        const auto t3 = std::chrono::steady_clock::now();
        pc.add("5 reads pack+upload", std::chrono::duration<double>(t1 - t0).count());
        pc.add("6 map", std::chrono::duration<double>(t2 - t1a).count());
        pc.add("6a waited for the device", std::chrono::duration<double>(t1a - t1).count());
        pc.add("7 mapq+fetch+format", std::chrono::duration<double>(t3 - t2).count());
        if (sw.timing) { std::ostringstream os; os << "INFO, worker " << d << "." << wi << " batch " << seq << ": upload " << std::chrono::duration<double>(t1 - t0).count() << " map "
          << std::chrono::duration<double>(t2 - t1a).count() << " (waited " << std::chrono::duration<double>(t1a - t1).count() << "; device ms: K1 " << gst.ms_minimizer << " K2 " << gst.ms_sketch << " K3 " << gst.ms_probe_gather << " K4 " << gst.ms_sort_hits + gst.ms_l1_scan << " K5 " << gst.ms_l2 << " all " << gst.ms_total << ") finish " << std::chrono::duration<double>(t3 - t2).count() << " (mapq " << dn->t_mapq << " fetch " << dn->t_fetch << " format " << dn->t_format << ") done at +" << std::chrono::duration<double>(t3 - pc.t0).count() << " s\n"; std::cerr << os.str(); }
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
    struct Held { size_t file = 0; std::vector<std::string> names; std::vector<int> lens, clens /* --hpc: compressed */; std::vector<mm_seqset*> reads;
                  std::vector<mm_mapping*> sk;                 // per device: the batch's minimizers + sketches (mm_sketch_batch), computed once for all chunks
                  std::vector<mm_mapping*> part;               // per chunk: the batch's records against that chunk, on the device that holds the chunk (c mod G)
                  std::vector<std::vector<int64_t>> poff; std::vector<std::vector<mm_map_record>> prec; };   // --host-gather: the same in host memory (rounds 1-3)
    // How the records of a batch reach the device that merges them (unifyFiles, mapWrap.h:128-145, in place of the PREFIX.N files):
    //   rccl  (several physical devices) mm_mapping_gather: ncclSend / ncclRecv over xGMI, one collective per batch
    //   peer  (logical devices of one GPU, or --peer-gather) mm_mapping_concat pulls the parts of other contexts with device-to-device copies
    //   host  (--host-gather) mm_mapping_fetch + mm_mapping_from_parts: through host memory, the path of rounds 1-3, kept as the cross-check
    bool distinct = true; for (size_t a = 0; a < G; ++a) for (size_t b2 = a + 1; b2 < G; ++b2) distinct = distinct && devs[a].phys != devs[b2].phys;
    enum class Gather { Rccl, Peer, Host } gather = o.v.count("host-gather") ? Gather::Host : (G > 1 && distinct && !o.v.count("peer-gather")) ? Gather::Rccl : Gather::Peer;
    if (sw.timing) std::cerr << "INFO, records of the chunks are gathered by " << (gather == Gather::Rccl ? "RCCL send / receive" : gather == Gather::Peer ? "device-to-device copies" : "the host") << "\n";
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
          ck(ctx, mm_mapping_gather(ctx, (int)(b % G), (int64_t)h.names.size(), (hpc ? h.clens : h.lens).data(), &mp, mine.data(), ids.data(), (int)mine.size(), (int)NC, chunk_rank.data(), chunk_base.data(), &m), "gather chunks");
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
    const size_t minReadsU = o.v.count("minreads") ? std::stoull(o.v.at("minreads")) : 10000;   // parseCmdArgs.hpp:462-471
    // the last prefix ends the process from inside classify_one, as the last file of `classify` does: everything is written and closed, the
    // gigabyte of line tables and text is not taken apart first (MM_CLI_FULL_TEARDOWN=1: the orderly way)
    const std::function<void()> leave = [&] { pc.lap("9 classify"); pc.report(); };
    for (size_t fi = 0; fi < prefixes.size(); ++fi) {
      const bool last = fi + 1 == prefixes.size();
      KeptLines kl; kl.cname = &cname;
      if (keep_lines && fi < kept.size()) for (const auto& d : kept[fi]) kl.parts.push_back(KeptLines::Part{d->text.data(), d->meta.data(), d->meta.size(), d->off.data(), d->lens.size()});
      classify_one(devs, reduce, prefixes[fi], o.v.at("then-classify"), minReadsU, last ? leave : std::function<void()>(), nullptr, keep_lines ? &kl : nullptr, boot_options(o), lca_options(o), gene_options(o), ident_options(o), sw);
      if (keep_lines && fi < kept.size()) kept[fi].clear();
      for (auto& d : devs) mm_comm_destroy(d.ctx);
      pc.lap("9 classify");
    }
  }

  int run() {
    read_parameters();
    open_devices();
    if (!from_index) {
      load_reference();
      plan_chunks();
      if (only_index) return write_index_files();
    } else read_index_files();
    decide_placement();
    build_resident_indexes();
    mp = mm_map_params{k, w, pi, minLen};
    for (auto& ch : chunks) chunk_base.push_back(ch.first);
    if (bam) bam_head = bam_header_members(ctx0, cname, clen);    // (before the workers take the first device's context)
    start_reader();
    if (prewarm.joinable()) prewarm.join();
    if (place != Place::Replicated) for (auto*& c : wctx) if (c) { mm_ctx_destroy(c); c = nullptr; }   // (the other modes drive one context per device)
    if (place == Place::Replicated) run_replicated(); else run_chunk_major();
    pc.lap("8 write");
    then_classify();
    if (!sw.full_teardown) { if (reader.th.joinable()) reader.th.join(); pc.report(); finish_fast(); }
    drop_refsets();
    for (auto& d : devs) { for (auto* ix : d.idx) if (ix) mm_index_destroy(ix); mm_ctx_destroy(d.ctx); }
    return 0;
  }
};

int map_mode(const Options& o, const std::string& mode, const CliSwitches& sw) { MapRun run(o, mode, sw); return run.run(); }

}  // namespace
