// `classify`: the EM over the devices (run_em_sharded) and one run of one mappings file (ClassifyRun), with the form in which mapDirectly
// --then-classify hands its lines over in memory (LineMeta, KeptLines).
#pragma once
#include "bam_reader.hpp"
#include "cli_device.hpp"
#include "cli_switches.hpp"
#include "gene_annot.hpp"
#include "ident_filter.hpp"
#include "query_reader.hpp"
#include "taxonomy.hpp"
#include <fcntl.h>
#include <sys/mman.h>
#include <climits>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <unordered_map>

namespace {

// A mapping line as `classify` sees it once it has tokenised the file (fEM.h:234-275): where the line lies in the text, and the values of the fields it reads
// — identity and mapping quality as the PRINTED text parses, not as the floats they were printed from.  `mapDirectly --then-classify` keeps these beside the
// text it writes, so that classify in the same process neither reads the file back nor tokenises it.
struct LineMeta {
  uint32_t beg, ls /* the blank before field 14, relative to beg */, n /* length without the newline */;
  int32_t contig /* index into the reference's contigs */, len, start, stop /* field 9: start + len - 1, or its raw translation with --hpc */;
  double ident, mapq;
};
enum class EmReduce { None, Rccl, Host };
struct KeptLines {                                               // the mapping lines of one output prefix as mapDirectly wrote them, batch after batch, with their parsed fields
  struct Part { const char* text; const LineMeta* meta; size_t n_lines; const int64_t* off; size_t n_reads; };
  std::vector<Part> parts; const std::vector<std::string>* cname = nullptr;
};

// ------------------------------------------------------------------------------------------------------
// The EM loop of classify across devices (meta::doEM, fEM.h:501-661).  The reads are sharded contiguously — rank order = read
// order, as the reference shards them over OpenMP threads (:1229) —, every rank computes the per-taxon posterior sums and the
// log-likelihood of its reads, the sums of the ranks are added (the merge of the per-thread sums, :583-600), and every rank
// normalises and evaluates the stop rule (:624-639) on identical values.
//   Rccl  one ncclAllReduce(f64, T+1) per iteration inside the device-resident loop (mm_em_run / mm_em_continue): the production path
//   Host  each rank's partial sums (mm_em_iterate) added on the host in rank order — what the all-reduce delivers —; several ranks
//         may then share one device, which is how everything AROUND the collective is tested on a one-GPU box (--em-host-reduce)
//   None  one rank, no communicator
struct EmShard { size_t lo = 0, hi = 0, e0 = 0; std::vector<int64_t> soff; };   // reads [lo, hi); e0: first mapping of the shard; soff: shard-local offsets
EmShard em_shard(const std::vector<int64_t>& off, size_t G, size_t d) {
  const size_t NR = off.size() - 1, base = NR / G, rem = NR % G;
  EmShard s;
  s.lo = d * base + std::min(d, rem); s.hi = s.lo + base + (d < rem ? 1 : 0);
  s.e0 = (size_t)off[s.lo];
  s.soff.resize(s.hi - s.lo + 1);
  for (size_t i = 0; i <= s.hi - s.lo; ++i) s.soff[i] = off[s.lo + i] - off[s.lo];
  return s;
}
struct ThreadBarrier {
  std::mutex m; std::condition_variable cv; const size_t n; size_t waiting = 0, gen = 0;
  explicit ThreadBarrier(size_t n_) : n(n_) {}
  void wait() { std::unique_lock<std::mutex> lk(m); const size_t g = gen; if (++waiting == n) { waiting = 0; ++gen; cv.notify_all(); } else cv.wait(lk, [&] { return gen != g; }); }
};
void print_em_round(long long it, double ll, double ll_prev) {  // the per-round lines of the reference's log (fEM.h:503, :602-603, :631-632)
  std::cout << "EM round " << it << std::endl << "\n\tLog likelihood: " << ll << std::endl;
  if (it > 0) std::cout << "\tImprovement: " << ll - ll_prev << "\n\tRelative   : " << ll / ll_prev << std::endl;
}
// f: start frequencies in, final frequencies out; post[mapping], best[read] (index into the whole mapping list) out; lca (may be null): every
// rank's reads assigned behind its posteriors, the ranks' direct counts added; rounds (may be null): the EM rounds that were run
void run_em_sharded(const std::vector<Dev>& devs, EmReduce reduce, const std::vector<int64_t>& off, const std::vector<int32_t>& taxon,
                    const std::vector<double>& mapq, const std::vector<double>& inv, size_t NT, std::vector<double>& f,
                    std::vector<double>& post, std::vector<int64_t>& best, LcaJob* lca, const CliSwitches& sw, long long* rounds = nullptr) {
  const size_t G = devs.size();
  if (reduce == EmReduce::None && G != 1) die("internal error: several EM ranks without a reduction");
  char comm_id[MM_COMM_ID_BYTES];
  if (reduce == EmReduce::Rccl && mm_comm_unique_id(comm_id) != MM_OK) die("RCCL: cannot create a communicator id");
  const std::vector<double> f0 = f;
  std::vector<std::vector<double>> part(G, std::vector<double>(NT + 1, 0.0));   // Host: the ranks' partial sums of one iteration
  std::vector<double> f_cur = f0; bool host_stop = false; double ll_prev = 0;
  ThreadBarrier bar(G);
  const long long MAX_ITER = sw.em_max_iter;
  const int SLICE = sw.em_slice;
  on_each(G, [&](size_t d) {
    mm_ctx* ctx = devs[d].ctx;
    if (reduce == EmReduce::Rccl) ck(ctx, mm_comm_init(ctx, comm_id, (int)d, (int)G), "RCCL communicator");
    const EmShard sh = em_shard(off, G, d);
    const size_t n = sh.hi - sh.lo;
    mm_em* em; ck(ctx, mm_em_create(ctx, (int64_t)n, sh.soff.data(), taxon.data() + sh.e0, mapq.data() + sh.e0, inv.data() + sh.e0, (int32_t)NT, &em), "em");
    std::vector<double> fl(NT);
    if (reduce != EmReduce::Host) {
      // the loop itself runs on the device (E step, sums, all-reduce, normalisation and the stop rule per iteration, no host round
      // trip), in slices of <= 1024 iterations so that every round's log-likelihood reaches the log as in the reference
      std::vector<double> lls((size_t)std::min(SLICE, 1024));
      long long done = 0; double prev = 0;
      for (bool first = true;; first = false) {
        int n_iter = 0, stopped = 0;
        const int want = (int)std::min<long long>((long long)lls.size(), MAX_ITER - done);
        if (want <= 0) break;
        if (first) { ck(ctx, mm_em_run(em, f0.data(), want, fl.data(), lls.data(), (int)lls.size(), &n_iter), "em"); stopped = n_iter < want; }
        else ck(ctx, mm_em_continue(em, want, fl.data(), lls.data(), (int)lls.size(), &n_iter, &stopped), "em");
        if (d == 0) for (int it = 0; it < n_iter; ++it) { print_em_round(done + it, lls[(size_t)it], prev); prev = lls[(size_t)it]; }
        done += n_iter;
        if (stopped || n_iter == 0) break;
      }
      if (d == 0 && rounds) *rounds = done;
    } else {
      for (long long it = 0; it < MAX_ITER; ++it) {
        ck(ctx, mm_em_iterate(em, f_cur.data(), part[d].data(), &part[d][NT]), "em");
        bar.wait();
        if (d == 0) {                                            // the sum over the ranks, in rank order; normalisation (fEM.h:606-615); stop rule (:624-639)
          std::vector<double> tot(NT + 1, 0.0);
          for (size_t g = 0; g < G; ++g) for (size_t t = 0; t <= NT; ++t) tot[t] += part[g][t];
          double sum = 0; for (size_t t = 0; t < NT; ++t) sum += tot[t];
          for (size_t t = 0; t < NT; ++t) f_cur[t] = tot[t] / sum;
          const double ll = tot[NT];
          print_em_round(it, ll, ll_prev);
          if (rounds) *rounds = it + 1;
          if (it > 0 && (ll - ll_prev) <= 1 && (1 - ll / ll_prev) < 0.0001) host_stop = true;
          ll_prev = ll;
        }
        bar.wait();
        if (host_stop) break;
      }
      fl = f_cur;
    }
    std::vector<int64_t> bl(n);
    ck(ctx, mm_em_posteriors(em, fl.data(), post.data() + sh.e0, bl.data()), "posteriors");
    for (size_t i = 0; i < n; ++i) best[sh.lo + i] = bl[i] < 0 ? -1 : bl[i] + (int64_t)sh.e0;   // rank-local index -> index into the whole mapping list
    if (lca) {
      std::vector<int64_t> dl(lca->id.size());
      ck(ctx, mm_em_lca(em, fl.data(), (int32_t)lca->id.size(), lca->parent.data(), lca->taxon_node.data(), lca->tau, lca->node.data() + sh.lo, lca->mass.data() + sh.lo, dl.data()), "lca");
      std::lock_guard<std::mutex> lk(lca->m);
      for (size_t v = 0; v < dl.size(); ++v) lca->direct[v] += dl[v];
    }
    mm_em_destroy(em);
    bar.wait();                                                  // (every rank has read f_cur)
    if (d == 0) f = fl;
  });
}

// One `classify` of one mappings file (meta::doEM, fEM.h:466-803): the file read and tokenised, the database's tables, the EM on the devices, every output
// file.  The stages are the methods, in the order run() calls them.  (Until round 5 one 280-line function.)
struct ClassifyRun {
  const std::vector<Dev>& devs; const EmReduce reduce; const std::string& mapped; const std::string& db; const size_t minReadsU;
  const std::function<void()>& leave_now;      // the last file: called once everything is written; the process ends there (may be empty)
  const std::function<void()>& need_devices;   // called before the first device call: the contexts are created beside the parsing of the file (may be empty)
  const CliSwitches& sw;
  PhaseClock pc{sw.timing};
  const unsigned HW = mm::cpu_budget();                        // CPUs this process may keep busy (cpu_budget.hpp: a container's quota counts, not the 256 the machine shows)
  const unsigned WIDE = std::max(1u, HW - std::max(1u, HW / 8));   // width of the pools that compute flat out: under a CPU quota (16 CPUs' worth of time per 100 ms) sixteen such threads plus
                                                               // whatever else runs use the period up, and every thread of the process is stopped for the rest of it (bench: c1 0.11 -> 0.21 s)
  struct TextBuf {                                               // the file's bytes + a terminating 0, not zero-filled first (std::string::resize spent 0.1 s on that per 0.5 GB)
    char* p = nullptr; size_t n = 0;
    void resize(size_t k) { p = new (std::nothrow) char[k + 1]; if (!p) die("out of host memory for the mappings file"); n = k; p[k] = 0; }   // (huge_new.hpp: on huge pages)
    size_t size() const { return n; } const char* c_str() const { return p; } char& operator[](size_t i) { return p[i]; }
    ~TextBuf() { delete[] p; }
  };
  TextBuf text;
  struct MapLine { const char* p; uint32_t last_space, n; int contig; long long len; size_t start, stop; double ident, mapq; };   // [p, p + n): the line; p + last_space: the blank before field 14
  const KeptLines* kept = nullptr;                                // mapDirectly --then-classify: the lines in memory (no file is read)
  std::vector<MapLine> lines; std::vector<int64_t> off{0};       // read r owns lines [off[r], off[r+1])
  std::vector<std::string> contig_id; std::unordered_map<std::string, int> contig_index;
  size_t NRD = 0;
  std::vector<std::string> contig_taxon_id; std::set<std::string> taxaSet;
  std::map<std::string, size_t> st; size_t nUnmapped = 0, nTooShort = 0, nTotal = 0;
  std::map<std::string, std::map<std::string, size_t>> TI;       // fEM.h:1320-1364
  std::unique_ptr<Taxonomy> tax;
  std::vector<std::string> taxa;
  std::vector<int> contig_tx; std::vector<long long> contig_len_ti;   // per contig: taxon index; length per taxonInfo (-1: not listed)
  std::vector<int32_t> taxon; std::vector<double> mapq, inv;          // per mapping
  std::vector<double> f, post; std::vector<int64_t> best;
  BootOpts boot;                                                  // --bootstrap: the replicates' frequencies of the present taxa, [replicate][boot_pres]
  std::vector<int32_t> boot_pres; std::vector<double> boot_f;
  std::vector<char> boot_empty;                                   // [replicate]: it drew no read (mm_em_bootstrap: n_iter == 0) and has no estimate
  LcaOpts lca; std::unique_ptr<LcaJob> lca_job;                   // --lca
  GeneOpts genes;                                                 // --genes
  IdentOpts identf_opts;                                          // --min-identity, --refit

  ClassifyRun(const std::vector<Dev>& devs_, EmReduce reduce_, const std::string& mapped_, const std::string& db_, size_t minReadsU_, const std::function<void()>& leave_now_,
              const std::function<void()>& need_devices_, const CliSwitches& sw_)
      : devs(devs_), reduce(reduce_), mapped(mapped_), db(db_), minReadsU(minReadsU_), leave_now(leave_now_), need_devices(need_devices_), sw(sw_) {}

  // The mappings file once through: every line is tokenised where it lies (the reference splits every line again in every EM round,
  // fEM.h:1171-1214, :234-373), lines of one read are consecutive (mapWrap.h:128-149), contig IDs are interned.
  // Round 4: read and tokenised by several threads — pieces of the file that begin on a read boundary are parsed on their own and joined in
  // file order (read offsets shifted, contig IDs interned in the order a single pass would meet them): 4.2 M lines took 1.3 s on one thread.
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
    if (need_devices) need_devices();
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
    {
      const int fd = ::open(src.c_str(), O_RDONLY);
      if (fd < 0) die("Cannot open mappings file " + mapped);
      struct stat stt; if (fstat(fd, &stt) != 0) die("Cannot open mappings file " + mapped);
      text.resize((size_t)stt.st_size);
      const size_t PIECE = (size_t)32 << 20, np = (text.size() + PIECE - 1) / PIECE;
      std::atomic<size_t> nx{0}; std::atomic<bool> bad{false};
      auto rd = [&] { for (;;) { const size_t i = nx.fetch_add(1); if (i >= np) return; size_t a0 = i * PIECE; const size_t e0 = std::min(text.size(), a0 + PIECE);
                        while (a0 < e0) { const ssize_t g = pread(fd, &text[a0], e0 - a0, (off_t)a0); if (g <= 0) { bad = true; return; } a0 += (size_t)g; } } };
      std::vector<std::thread> pool; for (unsigned t = 1; t < std::min<unsigned>({8u, HW, (unsigned)std::max<size_t>(np, 1)}); ++t) pool.emplace_back(rd);
      rd(); for (auto& t : pool) t.join();
      ::close(fd);
      if (bad) die("Cannot read mappings file " + mapped);
    }
  }
  void tokenise() {
    {
      const char* const T0 = text.c_str();
      const size_t TS = text.size();
      // the read ID of the line that starts at p (text up to the first blank or the line's end)
      auto id_of = [&](size_t p, size_t& len) { const char* nl = (const char*)memchr(T0 + p, '\n', TS - p); const size_t e = nl ? (size_t)(nl - T0) : TS;
                                                const char* sp = (const char*)memchr(T0 + p, ' ', e - p); len = (sp ? (size_t)(sp - T0) : e) - p; };
      auto next_line = [&](size_t p) { const char* nl = (const char*)memchr(T0 + p, '\n', TS - p); return nl ? (size_t)(nl - T0) + 1 : TS; };
      // first read boundary at or after x: a line start whose ID differs from the ID of the last non-empty line before it
      auto read_boundary = [&](size_t x) {
        if (x == 0) return (size_t)0;
        size_t p = next_line(x - 1);                                // start of the first line that begins at or after x
        while (p < TS) {
          if (T0[p] == '\n') { ++p; continue; }                     // empty line
          size_t q = p;                                            // start of the previous non-empty line
          for (;;) { if (q == 0) return p; size_t e = q - 1; size_t b0 = e; while (b0 > 0 && T0[b0 - 1] != '\n') --b0; if (e > b0) { q = b0; break; } q = b0; }
          size_t la, lb; id_of(p, la); id_of(q, lb);
          if (la != lb || memcmp(T0 + p, T0 + q, la) != 0) return p;
          p = next_line(p);
        }
        return TS;
      };
      // (MM_CLASSIFY_THREADS=n: exactly n pieces, whatever the size of the file — the tests cut small files into many)
      const size_t NTH = sw.classify_threads ? (size_t)sw.classify_threads
                                                       : std::max<size_t>(1, std::min<size_t>({(size_t)32, (size_t)WIDE, TS / ((size_t)4 << 20) + 1}));
      std::vector<size_t> cut(NTH + 1, TS);
      cut[0] = 0;
      for (size_t t = 1; t < NTH; ++t) cut[t] = std::max(cut[t - 1], read_boundary(TS / NTH * t));
      struct Piece { std::vector<MapLine> lines; std::vector<int64_t> starts; std::vector<std::string> cid; std::unordered_map<std::string, int> cix; };
      std::vector<Piece> pieces(NTH);
      auto parse_piece = [&](size_t t) {
        Piece& P = pieces[t];
        size_t cur_beg = 0, cur_len = (size_t)-1;                  // the current read's ID, as a span of `text`
        for (size_t p = cut[t]; p < cut[t + 1];) {
          const char* nl = (const char*)memchr(T0 + p, '\n', cut[t + 1] - p);
          const size_t e = nl ? (size_t)(nl - T0) : cut[t + 1];
          if (e == p) { p = e + 1; continue; }                     // empty line
          size_t fb[16], fe[16]; int nf = 0;                       // fields (single blanks, util.h:80)
          for (size_t q = p; nf < 16;) { const char* sp = (const char*)memchr(T0 + q, ' ', e - q); fb[nf] = q; fe[nf] = sp ? (size_t)(sp - T0) : e; ++nf; if (!sp) break; q = fe[nf - 1] + 1; }
          if (nf < 6) die("File " + mapped + " has weird format - is this a mappings file generated by MetaMap?");
          if (nf < 14) die("File " + mapped + " has lines with fewer than 14 fields - is this a mappings file generated by MetaMap?");
          if (fe[0] - fb[0] != cur_len || memcmp(T0 + fb[0], T0 + cur_beg, cur_len) != 0) { P.starts.push_back((int64_t)P.lines.size()); cur_beg = fb[0]; cur_len = fe[0] - fb[0]; }
          MapLine L{};
          L.p = T0 + p; L.n = (uint32_t)(e - p); L.last_space = (uint32_t)(fb[13] - 1 - p);
          std::string cid(T0 + fb[5], fe[5] - fb[5]);
          auto it = P.cix.find(cid);
          if (it == P.cix.end()) { it = P.cix.emplace(cid, (int)P.cid.size()).first; P.cid.push_back(cid); }
          L.contig = it->second;
          L.len = strtoll(T0 + fb[1], nullptr, 10);
          L.start = strtoull(T0 + fb[7], nullptr, 10); L.stop = strtoull(T0 + fb[8], nullptr, 10);
          L.ident = strtod(T0 + fb[9], nullptr) / 100.0;
          { errno = 0; char* endp = nullptr; L.mapq = strtod(T0 + fb[13], &endp);   // std::stod: out of range (also a denormal) throws; the reference then takes 0 for "…e-…" (fEM.h:269-275)
            if (errno == ERANGE) { if (std::string(T0 + fb[13], fe[13] - fb[13]).find("e-") != std::string::npos) L.mapq = 0; else die("mapping quality out of range in " + mapped); }
            if (endp == T0 + fb[13]) die("File " + mapped + " has a mapping quality that is not a number"); }
          P.lines.push_back(L);
          p = e + 1;
        }
      };
      { std::vector<std::thread> pool; for (size_t t = 1; t < NTH; ++t) pool.emplace_back(parse_piece, t); parse_piece(0); for (auto& th : pool) th.join(); }
      // join: contig IDs in the order of their first line, read offsets shifted by the lines before the piece
      std::vector<std::vector<int>> remap(NTH);
      std::vector<size_t> line0(NTH + 1, 0);
      for (size_t t = 0; t < NTH; ++t) {
        line0[t + 1] = line0[t] + pieces[t].lines.size();
        remap[t].resize(pieces[t].cid.size());
        for (size_t c = 0; c < pieces[t].cid.size(); ++c) {
          auto it = contig_index.find(pieces[t].cid[c]);
          if (it == contig_index.end()) { it = contig_index.emplace(pieces[t].cid[c], (int)contig_id.size()).first; contig_id.push_back(pieces[t].cid[c]); }
          remap[t][c] = it->second;
        }
      }
      lines.resize(line0[NTH]);
      off.clear();
      for (size_t t = 0; t < NTH; ++t) for (int64_t st0 : pieces[t].starts) off.push_back(st0 + (int64_t)line0[t]);
      if (off.empty()) off.push_back(0);
      auto place = [&](size_t t) {
        MapLine* o = lines.data() + line0[t]; const auto& src = pieces[t].lines;
        for (size_t i = 0; i < src.size(); ++i) { o[i] = src[i]; o[i].contig = remap[t][(size_t)src[i].contig]; }
      };
      { std::vector<std::thread> pool; for (size_t t = 1; t < NTH; ++t) pool.emplace_back(place, t); place(0); for (auto& th : pool) th.join(); }
      if (!lines.empty()) off.push_back((int64_t)lines.size());
    }
    NRD = off.size() - 1;
  }
  // the taxa of the mapped contigs, PREFIX.meta, DB/taxonInfo.txt
  void read_tables() {
    contig_taxon_id.assign(contig_id.size(), std::string());
    for (size_t c = 0; c < contig_id.size(); ++c) { contig_taxon_id[c] = extract_taxon(contig_id[c]); taxaSet.insert(contig_taxon_id[c]); }
    if (taxaSet.empty()) die("No relevant taxon IDs found in your mappings file - is it possible that none of your reads are mapped?");
    { std::ifstream s(mapped + ".meta");
      if (!s.is_open()) die("The file " + mapped + ".meta is not present or could not be opened - this file is generated automatically as part of the "
                            "mapping process, so please check whether the mapping process finished successfully.");
      std::string a; size_t b; while (s >> a >> b) st[a] = b; }
    nUnmapped = st.at("ReadsNotMapped"); nTooShort = st.at("ReadsTooShort"); nTotal = st.at("TotalReads");
    { std::ifstream s(db + "/taxonInfo.txt"); if (!s.is_open()) die("Could not open file " + db + "/taxonInfo.txt -- perhaps you have specified an incomplete DB?");
      std::string ln;
      while (std::getline(s, ln)) {
        if (ln.empty()) continue;
        auto f = split(ln, " ");
        for (auto& c : split(f.at(1), ";")) { auto kv = split(c, "="); TI[f.at(0)][kv.at(0)] = std::stoull(kv.at(1)); }
      } }
  }
  void per_mapping_fields() {
    taxa.assign(taxaSet.begin(), taxaSet.end());
    std::map<std::string, int> tindex; for (size_t i = 0; i < taxa.size(); ++i) tindex[taxa[i]] = (int)i;
    // per mapping: taxon, quality, 1/nLoc (getMappingLocations, fEM.h:234-353).  nLoc(read, taxon) = sum over the taxon's contigs of
    // (len - L + 1) if len >= L, else 1 if the read has a mapping on that contig (:325-348): sorted lengths + suffix sums per taxon
    contig_tx.assign(contig_id.size(), 0); contig_len_ti.assign(contig_id.size(), -1);
    struct TaxLens { std::vector<long long> len, suffix; };
    std::vector<TaxLens> tl(taxa.size());
    for (size_t t = 0; t < taxa.size(); ++t) {
      auto it = TI.find(taxa[t]);
      if (it == TI.end()) die("Unknown taxonID '" + taxa[t] + "'; please check that your mappings file was mapped against the database now specified.");
      for (auto& c : it->second) tl[t].len.push_back((long long)c.second);
      std::sort(tl[t].len.begin(), tl[t].len.end());
      tl[t].suffix.assign(tl[t].len.size() + 1, 0);
      for (size_t i = tl[t].len.size(); i-- > 0;) tl[t].suffix[i] = tl[t].suffix[i + 1] + tl[t].len[i];
    }
    for (size_t c = 0; c < contig_id.size(); ++c) {
      contig_tx[c] = tindex.at(contig_taxon_id[c]);
      auto& m = TI.at(contig_taxon_id[c]); auto it = m.find(contig_id[c]);
      if (it != m.end()) contig_len_ti[c] = (long long)it->second;
    }
    taxon.assign(lines.size(), 0); mapq.assign(lines.size(), 0.0); inv.assign(lines.size(), 0.0);
    {
      std::vector<int> seen_c;                                     // distinct contigs of the current read
      for (size_t r = 0; r < NRD; ++r) {
        const size_t a0 = (size_t)off[r], b0 = (size_t)off[r + 1];
        const long long L = lines[a0].len;
        seen_c.clear();
        for (size_t i = a0; i < b0; ++i) if (std::find(seen_c.begin(), seen_c.end(), lines[i].contig) == seen_c.end()) seen_c.push_back(lines[i].contig);
        for (size_t i = a0; i < b0; ++i) {
          const int t = contig_tx[(size_t)lines[i].contig];
          const TaxLens& X = tl[(size_t)t];
          const size_t k0 = (size_t)(std::lower_bound(X.len.begin(), X.len.end(), L) - X.len.begin());
          long long n = X.suffix[k0] - (long long)(X.len.size() - k0) * (L - 1);
          for (int c : seen_c) if (contig_tx[(size_t)c] == t && contig_len_ti[(size_t)c] >= 0 && contig_len_ti[(size_t)c] < L) ++n;
          taxon[i] = t; mapq[i] = lines[i].mapq; inv[i] = 1 / (double)(size_t)n;
        }
      }
    }
  }
  void em() {
    const size_t NT = taxa.size(), NR = NRD;
    f.assign(NT, 1 / (double)NT);
    post.assign(taxon.size(), 0.0); best.assign(NR, 0);
    std::cout << "Starting EM..." << std::endl;
    if (need_devices) need_devices();
    if (lca.on) lca_job = std::make_unique<LcaJob>(*tax, taxa, lca.tau, NR);
    run_em_sharded(devs, reduce, off, taxon, mapq, inv, NT, f, post, best, lca_job.get(), sw);
  }
  // PREFIX.EM.reads2Taxon.lca: readID, taxon ID, rank and mass of the LCA assignment of every read with a mapping, in the order of reads2Taxon
  void write_lca_reads(const std::string& fn) const {
    const LcaJob& J = *lca_job;
    std::string out; char num[48];
    for (size_t r = 0; r < NRD; ++r) {
      const MapLine& B = lines[(size_t)off[r]];
      const std::string& id = J.id[(size_t)J.node[r]];
      out.append(B.p, (size_t)((const char*)memchr(B.p, ' ', B.n) - B.p)); out += '\t'; out += id; out += '\t'; out += tax->T.at(id).rank;
      snprintf(num, sizeof num, "\t%.6f\n", J.mass[r]); out += num;
    }
    std::ofstream o(fn);
    o.write(out.data(), (std::streamsize)out.size());
  }
  // --genes: the best mappings of all reads against the annotated genes of their contigs, on the first device (mm_gene_overlap; medians do not merge
  // across shards, and the job is small); PREFIX.EM.geneLevelAnalysis and PREFIX.EM.proteins.TYPE beside the WIMP
  void gene_analysis() {
    std::unordered_map<std::string, int> relevant;                // contigs with a best mapping, in the order of their first one
    std::vector<int> rel_of(contig_id.size(), -1);
    std::vector<int32_t> mc(NRD), ms(NRD), me(NRD); std::vector<double> mi(NRD);
    for (size_t r = 0; r < NRD; ++r) {
      const MapLine& B = lines[(size_t)best[r]];
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
  // --bootstrap B: replicates 0..B-1 of the weighted EM (mm_em_bootstrap), started from the point estimate, dealt to the devices in contiguous
  // ranges; every device holds the whole EM problem and tiles its range to its free memory.  The result depends on neither.  A replicate that
  // drew no read (e^-n of them for n mapped reads: small samples only) has no estimate and is left out of every statistic.
  void bootstrap() {
    if (boot.B <= 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t NT = taxa.size(), G = devs.size(), B = (size_t)boot.B;
    { std::vector<char> has(NT, 0); for (int32_t t : taxon) has[(size_t)t] = 1; for (size_t t = 0; t < NT; ++t) if (has[t]) boot_pres.push_back((int32_t)t); }
    const size_t NP = boot_pres.size();
    boot_f.assign(B * NP, 0.0);
    boot_empty.assign(B, 0);
    const int MAX_ITER = 10000;
    std::atomic<long long> at_cap{0}; std::atomic<int> it_min{INT_MAX}, it_max{0};
    on_each(G, [&](size_t d) {
      const size_t lo = B * d / G, hi = B * (d + 1) / G;
      if (hi <= lo) return;
      mm_ctx* ctx = devs[d].ctx;
      mm_em* em; ck(ctx, mm_em_create(ctx, (int64_t)NRD, off.data(), taxon.data(), mapq.data(), inv.data(), (int32_t)NT, &em), "bootstrap");
      uint64_t tot = 0, fr = 0;
      ck(ctx, mm_ctx_device_info(ctx, nullptr, 0, nullptr, &tot, &fr), "device info");
      // per replicate on the device: posteriors (8 B per mapping), frequencies and sums (8 B per taxon, ~3x), a little per read block; half of
      // the free memory (the logical devices of one GPU share it); on the host the call's f_out (8 B per taxon) within 1 GiB
      const double per_rep = 8.0 * ((double)taxon.size() + 3.0 * (double)NT + (double)NRD / 64.0) + 1024.0;
      const size_t by_dev = (size_t)std::max(1.0, (double)fr / (2.0 * G) / per_rep), by_host = std::max<size_t>(1, ((size_t)1 << 30) / (8 * std::max<size_t>(NT, 1)));
      const size_t tile = std::max<size_t>(1, std::min({hi - lo, by_dev, by_host}));
      std::vector<double> fo(tile * NT), llo(tile); std::vector<int32_t> nit(tile), stp(tile);
      for (size_t r0 = lo; r0 < hi; r0 += tile) {
        const size_t n = std::min(tile, hi - r0);
        ck(ctx, mm_em_bootstrap(em, f.data(), (int32_t)r0, (int32_t)n, boot.seed, nullptr, MAX_ITER, fo.data(), llo.data(), nit.data(), stp.data()), "bootstrap");
        for (size_t k = 0; k < n; ++k) {
          for (size_t j = 0; j < NP; ++j) boot_f[(r0 + k) * NP + j] = fo[k * NT + (size_t)boot_pres[j]];
          if (nit[k] == 0) { boot_empty[r0 + k] = 1; continue; }
          if (!stp[k]) ++at_cap;
          int v = it_min.load(); while (nit[k] < v && !it_min.compare_exchange_weak(v, nit[k])) {}
          v = it_max.load(); while (nit[k] > v && !it_max.compare_exchange_weak(v, nit[k])) {}
        }
      }
      mm_em_destroy(em);
    });
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const size_t n_empty = (size_t)std::count(boot_empty.begin(), boot_empty.end(), (char)1);
    const std::string left_out = std::to_string(n_empty) + " of " + std::to_string(B) + " drew no read and are left out";
    if (B - n_empty < 2) die("--bootstrap: " + left_out + ": fewer than two replicates to describe");
    std::cout << "Bootstrap: " << B << " replicates, seed " << boot.seed << ", " << it_min.load() << "-" << it_max.load() << " EM iterations per replicate, "
              << secs << " s on " << G << " device(s)" << (n_empty ? ", " + left_out : std::string()) << std::endl;
    if (at_cap) std::cerr << "Warning: " << at_cap.load() << " of " << B << " bootstrap replicates reached " << MAX_ITER << " EM iterations without meeting the stop rule." << std::endl;
  }
  // PREFIX.EM.WIMP.bootstrap: the WIMP's rows without the -3 count rows, its EMFrequency text, and over the replicates (each through cleanF with
  // the point estimate's best-mapping tallies, then the WIMP's upward sums and per-level normalisation) mean, SD (n - 1), 2.5 % and 97.5 %
  // quantiles (linear between order statistics), n = the replicates that drew a read (bootstrap() has seen to n >= 2)
  void write_bootstrap(const std::string& fn, const Taxonomy& T, const std::map<std::string, double>& fmap, const std::map<std::string, size_t>& readsPer) {
    const size_t B = (size_t)boot.B, NP = boot_pres.size();
    UpMemo memo;
    const std::map<std::string, WimpLevel> W0 = wimp_em_frequencies(T, fmap, readsPer, &memo);
    struct Row { const std::string* L; std::string t; double em; std::vector<double> v; };
    std::vector<Row> rows;
    for (auto& lv : W0) {
      double emUnm = 0;
      for (auto& t : lv.second.keys) { if (t != "Undefined") rows.push_back(Row{&lv.first, t, lv.second.emF.at(t), {}}); else emUnm += lv.second.emF.at(t); }
      rows.push_back(Row{&lv.first, "0", emUnm, {}});
    }
    for (auto& R : rows) R.v.reserve(B);
    const double minF = 0.9 * (1.0 / (double)st.at("ReadsMapped"));
    for (size_t b = 0; b < B; ++b) {
      if (boot_empty[b]) continue;
      std::map<std::string, double> fm;                            // cleanF (fEM.h:1135-1163) of the replicate (taxa without a mapping: 0, dropped)
      for (size_t j = 0; j < NP; ++j) { const std::string& id = taxa[(size_t)boot_pres[j]]; const double v = boot_f[b * NP + j]; if (!(v < minF) || readsPer.count(id)) fm[id] = v; }
      double s = 0; for (auto& e : fm) s += e.second; for (auto& e : fm) e.second /= s;
      const std::map<std::string, WimpLevel> Wb = wimp_em_frequencies(T, fm, readsPer, &memo);
      for (auto& R : rows) {
        auto lv = Wb.find(*R.L);
        double v = 0;
        if (lv != Wb.end()) {
          if (R.t == "0") { auto u = lv->second.emF.find("Undefined"); if (u != lv->second.emF.end()) v = u->second; }
          else { auto e = lv->second.emF.find(R.t); if (e != lv->second.emF.end()) v = e->second; }
        }
        R.v.push_back(v);
      }
    }
    std::ofstream o(fn);
    o << "AnalysisLevel\ttaxonID\tName\tEMFrequency\tBootstrapMean\tBootstrapSD\tLower95\tUpper95\n";
    auto quantile = [](const std::vector<double>& x, double q) {   // numpy's default (linear)
      const double h = q * (double)(x.size() - 1); const size_t k = (size_t)std::floor(h);
      return k + 1 < x.size() ? x[k] + (h - (double)k) * (x[k + 1] - x[k]) : x[k];
    };
    char num[128];
    for (auto& R : rows) {
      const size_t n = R.v.size();
      double mean = 0; for (double v : R.v) mean += v; mean /= (double)n;
      double ss = 0; for (double v : R.v) ss += (v - mean) * (v - mean);
      std::vector<double> x = R.v; std::sort(x.begin(), x.end());
      snprintf(num, sizeof num, "\t%.6g\t%.6g\t%.6g\t%.6g\n", mean, std::sqrt(ss / (double)(n - 1)), quantile(x, 0.025), quantile(x, 0.975));
      o << *R.L << "\t" << R.t << "\t" << (R.t == "0" ? std::string("Unclassified") : T.T.at(R.t).sci) << "\t" << R.em << num;
    }
  }
  // a line of PREFIX.EM: the mapping line with field 14 replaced by std::to_string(posterior) (fEM.h:705)
  static void em_line(std::string& s, const MapLine& L, double p) { s.append(L.p, (size_t)L.last_space + 1); append_f6(s, p); s += '\n'; }
  // the lines PREFIX.EM.reads2Taxon ends in: the unmapped and the too short reads at taxon 0
  std::string unmapped_reads2taxon() const {
    std::string out, ln;
    std::ifstream s(mapped + ".meta.unmappedReadsLengths");
    while (std::getline(s, ln)) { if (ln.empty()) continue; out += split(ln, "\t").at(1); out += "\t0\n"; }
    return out;
  }
  static void write_text(const std::string& fn, const std::string& text) { std::ofstream o(fn); o.write(text.data(), (std::streamsize)text.size()); }
  // --min-identity T: the genomes whose best mappings have a median identity below 100 T are removed, on the first device for all reads (mm_ident_filter;
  // medians do not merge across shards); PREFIX.extractedIdentities and PREFIX.EM-filtered{,.reads2Taxon,.WIMP} beside the WIMP
  void identity_filter() {
    identf::Filter F;
    F.thr = identf_opts.T * 100.0;                                 // (the script's $identityThreshold *= 100)
    const size_t NT = taxa.size(), NE = lines.size();
    F.ident.resize(NE);
    for (size_t i = 0; i < NE; ++i) F.ident[i] = identf::identity_value(lines[i].p, lines[i].last_space);
    F.sorted_max.resize(NRD); F.taxon_reads.resize(NT); F.taxon_median.resize(NT); F.taxon_removed.resize(NT); F.read_removed.resize(NRD);
    if (identf_opts.refit) { F.read_src.resize(NRD); F.entry_src.resize(NE); F.read_off_out.resize(NRD + 1); }
    mm_ctx* const ctx = devs[0].ctx;
    const bool rf = identf_opts.refit;
    ck(ctx, mm_ident_filter(ctx, (int64_t)NRD, off.data(), taxon.data(), F.ident.data(), best.data(), (int32_t)NT, F.thr, F.sorted_max.data(), &F.n_with, &F.n_le,
                            F.taxon_reads.data(), F.taxon_median.data(), F.taxon_removed.data(), F.read_removed.data(), rf ? F.read_src.data() : nullptr,
                            rf ? F.entry_src.data() : nullptr, rf ? F.read_off_out.data() : nullptr, rf ? &F.n_reads_out : nullptr, rf ? &F.n_entries_out : nullptr),
       "identity filter");
    F.sorted_max.resize((size_t)F.n_with);
    identf::write_identities(mapped + ".extractedIdentities", F, off, lines);
    std::string em, r2;
    std::vector<int64_t> kept(NT, 0);
    for (size_t r = 0; r < NRD; ++r) {
      const size_t b = (size_t)best[r];
      const MapLine& B = lines[b];
      r2.append(B.p, (size_t)((const char*)memchr(B.p, ' ', B.n) - B.p)); r2 += '\t';
      if (F.read_removed[r]) r2 += '0';
      else { r2 += taxa[(size_t)taxon[b]]; em_line(em, B, post[b]); kept[(size_t)taxon[b]]++; }
      r2 += '\n';
    }
    write_text(mapped + ".EM-filtered", em);
    write_text(mapped + ".EM-filtered.reads2Taxon", r2 + unmapped_reads2taxon());
    identf::write_filtered_wimp(mapped + ".EM-filtered.WIMP", *tax, taxa, kept, F.reads_removed(), nUnmapped, (size_t)F.n_with);
    char msg[256];
    snprintf(msg, sizeof msg, "Identity filter: threshold %g, median identity %g, %lld of %lld best identities at or below it, %zu of %zu genomes removed, %zu reads set to unclassified",
             F.thr, F.n_with ? F.sorted_max[(size_t)F.n_with / 2] : 0.0, (long long)F.n_le, (long long)F.n_with, F.genomes_removed(), F.genomes_hit(), F.reads_removed());
    std::cout << msg << std::endl;
    if (rf) identity_refit(F);
  }
  // --refit: the EM again on the mappings of the genomes that stay, from the flat start of em() and over the same devices; PREFIX.EM-filtered.refit (the
  // kept lines with their new posteriors), .refit.reads2Taxon (a read that lost every mapping: 0) and .refit.WIMP (such reads count as unmapped)
  void identity_refit(identf::Filter& F) {
    const size_t NT = taxa.size(), NR2 = (size_t)F.n_reads_out, NE2 = (size_t)F.n_entries_out, lost = (size_t)F.n_with - NR2;
    F.read_src.resize(NR2); F.entry_src.resize(NE2); F.read_off_out.resize(NR2 + 1);
    std::vector<int32_t> tx(NE2); std::vector<double> mq(NE2), iv(NE2);
    for (size_t k = 0; k < NE2; ++k) { const size_t e = (size_t)F.entry_src[k]; tx[k] = taxon[e]; mq[k] = mapq[e]; iv[k] = inv[e]; }
    std::vector<double> f2(NT, 1 / (double)NT), post2(NE2, 0.0); std::vector<int64_t> best2(NR2, 0);
    long long rounds = 0;
    if (NR2 > 0) {
      std::cout << "Starting EM on the filtered mappings..." << std::endl;
      if (reduce == EmReduce::Rccl) for (auto& d : devs) mm_comm_destroy(d.ctx);   // (run_em_sharded sets the communicator up)
      run_em_sharded(devs, reduce, F.read_off_out, tx, mq, iv, NT, f2, post2, best2, nullptr, sw, &rounds);
    }
    std::string em, r2;
    std::vector<size_t> readsPerIdx(NT, 0);
    size_t k = 0;                                                  // the next kept read
    for (size_t r = 0; r < NRD; ++r) {
      const MapLine& A = lines[(size_t)off[r]];
      r2.append(A.p, (size_t)((const char*)memchr(A.p, ' ', A.n) - A.p)); r2 += '\t';
      if (k < NR2 && (size_t)F.read_src[k] == r) {
        for (size_t j = (size_t)F.read_off_out[k]; j < (size_t)F.read_off_out[k + 1]; ++j) em_line(em, lines[(size_t)F.entry_src[j]], post2[j]);
        const size_t t = (size_t)tx[(size_t)best2[k]];
        r2 += taxa[t]; readsPerIdx[t]++; ++k;
      } else r2 += '0';
      r2 += '\n';
    }
    write_text(mapped + ".EM-filtered.refit", em);
    write_text(mapped + ".EM-filtered.refit.reads2Taxon", r2 + unmapped_reads2taxon());
    std::map<std::string, size_t> readsPer; std::map<std::string, double> fmap;
    for (size_t t = 0; t < NT; ++t) { if (readsPerIdx[t]) readsPer[taxa[t]] = readsPerIdx[t]; fmap[taxa[t]] = f2[t]; }
    { const double minF = 0.9 * (1.0 / (double)NR2); std::set<std::string> drop;   // cleanF (fEM.h:1135-1163) with the kept reads as ReadsMapped
      for (auto& e : fmap) if (e.second < minF && !readsPer.count(e.first)) drop.insert(e.first);
      for (auto& d : drop) fmap.erase(d);
      double s = 0; for (auto& e : fmap) s += e.second; for (auto& e : fmap) e.second /= s; }
    write_wimp(mapped + ".EM-filtered.refit.WIMP", *tax, fmap, readsPer, nTotal, nUnmapped + lost, nTooShort);
    std::cout << "Refit: " << NR2 << " reads, " << NE2 << " mappings, " << lost << " reads lost every mapping, " << rounds << " EM iterations" << std::endl;
  }
  void write_outputs() {
    Taxonomy& T = *tax;
    std::cout << "Outputting mappings with adjusted alignment qualities." << std::endl;
    std::ofstream emf(mapped + ".EM"), r2t(mapped + ".EM.reads2Taxon"), kr(mapped + ".EM.reads2Taxon.krona"), li(mapped + ".EM.lengthAndIdentitiesPerMappingUnit");
    li << "AnalysisLevel\tID\treadI\tIdentity\tLength\n";
    std::map<std::string, size_t> readsPer;
    ContigCoverage coverage;
    std::map<std::string, std::vector<double>> identsPerTaxon;     // :691, :718
    long long maxReadLen = -1;                                     // :692, :719-722
    std::thread side_files; bool unknown_written = true;
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } side_join{side_files};
    {
      // the four per-read / per-line files: ranges of reads formatted by several threads into their own buffers, written in read order
      // (4.2 M lines through std::to_string on one thread took 1.2 s); the per-taxon tallies and the coverage windows follow in read order
      std::vector<std::string> tax_nonx(taxa.size());              // getFirstNonXNode per taxon (taxonomy.h:51-74), once
      for (size_t t = 0; t < taxa.size(); ++t) tax_nonx[t] = T.first_non_x(taxa[t]);
      const size_t NTH = sw.classify_threads ? (size_t)sw.classify_threads
                                                       : std::max<size_t>(1, std::min<size_t>({(size_t)32, (size_t)WIDE, lines.size() / 50000 + 1}));
      std::vector<size_t> rcut(NTH + 1, NRD);
      rcut[0] = 0;
      { size_t t = 1; for (size_t r = 0; r < NRD && t < NTH; ++r) if ((uint64_t)off[r] >= (uint64_t)lines.size() * t / NTH) rcut[t++] = r; }
      struct Out { std::string em, r2, kr, li; };
      std::vector<Out> outs(NTH);
      auto fmt = [&](size_t t) {
        Out& O = outs[t];
        const size_t r0 = rcut[t], r1 = rcut[t + 1];
        if (r1 <= r0) return;
        { size_t bytes = 0; for (size_t i = (size_t)off[r0]; i < (size_t)off[r1]; ++i) bytes += lines[i].n + 5; O.em.reserve(bytes + 64); }
        char num[64];
        for (size_t r = r0; r < r1; ++r) {                         // fEM.h:684-779
          for (size_t i = (size_t)off[r]; i < (size_t)off[r + 1]; ++i) {   // the line with field 14 replaced by std::to_string(posterior) (:705)
            em_line(O.em, lines[i], post[i]);
          }
          const size_t b = (size_t)best[r];
          const MapLine& B = lines[b];
          const std::string& cg = contig_id[(size_t)B.contig];
          const size_t rid_len = (size_t)((const char*)memchr(B.p, ' ', B.n) - B.p);
          O.li += "EqualCoverageUnit\t"; O.li += cg; O.li += '\t';
          snprintf(num, sizeof num, "%zu\t%g\t%lld\n", r, B.ident, B.len); O.li += num;                  // :711
          O.r2.append(B.p, rid_len); O.r2 += '\t'; O.r2 += taxa[(size_t)taxon[b]]; O.r2 += '\n';
          O.kr.append(B.p, rid_len); O.kr += '\t'; O.kr += tax_nonx[(size_t)taxon[b]];
          snprintf(num, sizeof num, "\t%g\n", post[b]); O.kr += num;
        }
      };
      std::vector<std::thread> pool;
      for (size_t t = 1; t < NTH; ++t) pool.emplace_back(fmt, t);
      // meanwhile, on this thread: tallies per taxon and coverage windows, in read order (taxon and contig by index, strings only at the end)
      std::vector<size_t> readsPerIdx(taxa.size(), 0);
      std::vector<std::vector<double>> identsIdx(taxa.size());
      std::vector<ContigCoverage::Slot> cslot(contig_id.size());
      fmt(0);
      for (size_t r = 0; r < NRD; ++r) {                           // the window vectors of every contig with a best mapping (map insertions: one thread)
        const MapLine& B = lines[(size_t)best[r]];
        const size_t tx = (size_t)taxon[(size_t)best[r]];
        maxReadLen = std::max(maxReadLen, B.len);
        if (contig_len_ti[(size_t)B.contig] < 0) die("contig " + contig_id[(size_t)B.contig] + " is not listed for taxon " + taxa[tx] + " in " + db + "/taxonInfo.txt");
        ContigCoverage::Slot& sl = cslot[(size_t)B.contig];
        if (!sl.v) sl = coverage.slot(taxa[tx], contig_id[(size_t)B.contig], (size_t)contig_len_ti[(size_t)B.contig]);
      }
      {                                                            // tallies: thread k owns the taxa and the contigs with index % NT2 == k and walks the reads in order
        const size_t NT2 = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)std::max(1u, HW / 2), NRD / 20000 + 1}));
        auto tally = [&](size_t k) {
          for (size_t r = 0; r < NRD; ++r) {
            const size_t b = (size_t)best[r];
            const MapLine& B = lines[b];
            const size_t tx = (size_t)taxon[b];
            if (tx % NT2 == k) { readsPerIdx[tx]++; identsIdx[tx].push_back(B.ident); }
            if ((size_t)B.contig % NT2 == k) coverage.add(cslot[(size_t)B.contig], (size_t)contig_len_ti[(size_t)B.contig], B.start, B.stop);
          }
        };
        std::vector<std::thread> tp;
        for (size_t k = 1; k < NT2; ++k) tp.emplace_back(tally, k);
        tally(0);
        for (auto& th : tp) th.join();
      }
      for (size_t t = 0; t < taxa.size(); ++t) if (readsPerIdx[t]) { readsPer[taxa[t]] = readsPerIdx[t]; identsPerTaxon[taxa[t]] = std::move(identsIdx[t]); }
      for (auto& th : pool) th.join();
      pc.lap("c5a format");
      // the two side files only read the tallies, which are complete here: they are written beside the per-read files and the WIMP (0.1 s of their own)
      side_files = std::thread([&] {
        std::thread cov_thread([&] { coverage.write(mapped + ".EM.contigCoverage", T); });
        unknown_written = write_unknown_species(mapped + ".EM.evidenceUnknownSpecies", db, T, coverage, identsPerTaxon, maxReadLen, minReadsU);
        cov_thread.join();
      });
      auto put = [&](std::ofstream& f, std::string Out::*m) { for (auto& O : outs) f.write((O.*m).data(), (std::streamsize)(O.*m).size()); };
      std::thread w1([&] { put(r2t, &Out::r2); put(kr, &Out::kr); put(li, &Out::li); });
      put(emf, &Out::em);
      w1.join();
    }
    { std::ifstream s(mapped + ".meta.unmappedReadsLengths"); std::string ln;
      while (std::getline(s, ln)) { if (ln.empty()) continue; auto fl = split(ln, "\t"); r2t << fl.at(1) << "\t" << 0 << "\n"; kr << fl.at(1) << "\t" << 0 << "\t" << 0 << "\n"; } }
    std::map<std::string, double> fmap;
    for (size_t i = 0; i < taxa.size(); ++i) fmap[taxa[i]] = f[i];
    { const double minF = 0.9 * (1.0 / (double)st.at("ReadsMapped")); std::set<std::string> drop;   // cleanF, fEM.h:1135-1163
      for (auto& e : fmap) if (e.second < minF && !readsPer.count(e.first)) drop.insert(e.first);
      for (auto& d : drop) fmap.erase(d);
      double s = 0; for (auto& e : fmap) s += e.second; for (auto& e : fmap) e.second /= s; }
    pc.lap("c5 output files");
    write_wimp(mapped + ".EM.WIMP", T, fmap, readsPer, nTotal, nUnmapped, nTooShort);
    pc.lap("c6 WIMP");
    if (boot.B > 0) { write_bootstrap(mapped + ".EM.WIMP.bootstrap", T, fmap, readsPer); pc.lap("c6b WIMP bootstrap"); }
    if (lca.on) { write_lca_reads(mapped + ".EM.reads2Taxon.lca"); write_kreport(mapped + ".EM.kreport", T, *lca_job, nTotal, nUnmapped + nTooShort); pc.lap("c6c LCA files"); }
    if (genes.on) { gene_analysis(); pc.lap("c6d gene-level analysis"); }
    if (identf_opts.on) { identity_filter(); pc.lap("c6e identity filter"); }
    side_files.join();
    if (!unknown_written)
      std::cerr << "Warning: " << db << "/contigNstats_windowSize_1000.txt not found - " << mapped << ".EM.evidenceUnknownSpecies is not written." << std::endl;
    pc.lap("c8 evidence of unknown species + contig coverage");
    if (leave_now && !sw.full_teardown) { emf.close(); r2t.close(); kr.close(); li.close(); pc.report(); leave_now(); finish_fast(); }   // (a GB of vectors and strings: nothing left to do with them)
  }
  // mapDirectly --then-classify: the lines are in memory with their fields parsed (LineMeta) — what read_file + tokenise produce from the file, without the
  // file: read boundaries from the batches' offsets (reads without mappings have no lines), contig IDs interned in the order of their first line
  void adopt() {
    size_t total = 0; for (const auto& P : kept->parts) total += P.n_lines;
    lines.resize(total);
    off.clear();
    std::vector<int> intern(kept->cname->size(), -1);
    size_t at = 0;
    for (const auto& P : kept->parts) {
      for (size_t r = 0; r < P.n_reads; ++r) if (P.off[r + 1] > P.off[r]) off.push_back((int64_t)at + P.off[r]);
      for (size_t i = 0; i < P.n_lines; ++i) {
        const LineMeta& m = P.meta[i];
        int& ci = intern[(size_t)m.contig];
        if (ci < 0) { ci = (int)contig_id.size(); contig_id.push_back((*kept->cname)[(size_t)m.contig]); contig_index.emplace(contig_id.back(), ci); }
        lines[at + i] = MapLine{P.text + m.beg, m.ls, m.n, ci, (long long)m.len, (size_t)m.start, (size_t)m.stop, m.ident, m.mapq};
      }
      at += P.n_lines;
    }
    if (off.empty()) off.push_back(0);
    if (!lines.empty()) off.push_back((int64_t)lines.size());
    NRD = off.size() - 1;
  }
  int run() {
    if (kept) adopt(); else { read_file(); tokenise(); }
    read_tables();
    pc.lap("c1 read mappings + taxonInfo");
    tax = std::make_unique<Taxonomy>(db + "/taxonomy");
    pc.lap("c2 taxonomy");
    per_mapping_fields();
    pc.lap("c3 per-mapping fields");
    em();
    pc.lap("c4 EM");
    bootstrap();
    pc.lap("c4b EM bootstrap");
    write_outputs();
    return 0;
  }
};

int classify_one(const std::vector<Dev>& devs, EmReduce reduce, const std::string& mapped, const std::string& db, size_t minReadsU,
                 const std::function<void()>& leave_now, const std::function<void()>& need_devices, const KeptLines* kept, BootOpts boot, LcaOpts lca,
                 GeneOpts genes, IdentOpts identf_opts, const CliSwitches& sw) {
  ClassifyRun run(devs, reduce, mapped, db, minReadsU, leave_now, need_devices, sw);
  run.kept = kept;
  run.boot = boot;
  run.lca = lca;
  run.genes = genes;
  run.identf_opts = identf_opts;
  return run.run();
}

}  // namespace
