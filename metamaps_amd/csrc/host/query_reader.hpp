// The reader thread of mapDirectly / mapAgainstIndex: every query file in turn -> batches of reads in a bounded queue.  A file is BAM, bgzip text,
// plain gzip or plain text, by content (bam_reader.hpp); QueryReader has one method per kind and run() the bookkeeping they share.
#pragma once
#include "../../../include/metamaps_hip.h"
#include "../cpu_budget.hpp"
#include "bam_reader.hpp"
#include "cli_common.hpp"
#include "cli_switches.hpp"
#include "mods_out.hpp"
#include "seq_reader.hpp"
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>

namespace {

// a plain gzip file (starts with 1f 8b, not BGZF): what the device gzip reader takes unless MM_GZIP_HOST_INFLATE is set
bool is_plain_gzip_file(const std::string& path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  uint8_t b[2] = {0, 0};
  const ssize_t n = pread(fd, b, 2, 0);
  ::close(fd);
  return n == 2 && b[0] == 0x1f && b[1] == 0x8b && !bam::is_bgzf_file(path);
}

// A plain gzip file inflated on the device (mm_gzip_*, DESIGN.md §1 "Plain gzip on the device"), read in 64 MiB pieces: the `fill` source of
// a SeqFile, so the record parse is the zlib reader's byte for byte.  Corrupt data ends the program with the offset mm_last_error names.
struct DeviceGzip {
  mm_ctx* ctx; std::string path; FILE* f = nullptr; mm_gzip* g = nullptr;
  std::vector<uint8_t> piece; int64_t avail = 0; bool fed_last = false;
  DeviceGzip(mm_ctx* c, const std::string& p) : ctx(c), path(p), piece((size_t)64 << 20) {
    f = fopen(p.c_str(), "rb");
    if (!f) die("Cannot open " + p);
    if (mm_gzip_open(ctx, 0, 0, &g) != MM_OK) die(std::string("cannot open a device gzip stream: ") + mm_last_error(ctx));
  }
  ~DeviceGzip() { if (g) mm_gzip_close(g); if (f) fclose(f); }
  DeviceGzip(const DeviceGzip&) = delete;
  size_t fill(std::vector<unsigned char>& buf) {
    while (avail == 0 && !fed_last) {
      const size_t n = fread(piece.data(), 1, piece.size(), f);
      if (ferror(f)) die("Error reading " + path);
      fed_last = n < piece.size() && feof(f);
      const int rc = mm_gzip_feed(g, piece.data(), (int64_t)n, fed_last ? 1 : 0, &avail);
      if (rc == MM_ERR_DATA) die("Error reading " + path + ": " + mm_last_error(ctx));
      if (rc != MM_OK) die(std::string("device gzip inflate failed: ") + mm_last_error(ctx));
    }
    if (avail == 0) return 0;
    buf.resize((size_t)std::min<int64_t>(avail, (int64_t)64 << 20));
    int64_t got = 0;
    if (mm_gzip_read(g, buf.data(), (int64_t)buf.size(), &got) != MM_OK) die(std::string("device gzip read failed: ") + mm_last_error(ctx));
    avail -= got;
    return (size_t)got;
  }
};

// A batch's sequences live back to back in one arena (huge pages when the system grants them) that is handed to the library by
// reference (mm_seqset_add_view) and recycled: no allocation, copy or page fault per read.
struct Batch {
  std::vector<std::string> names; std::vector<int> lens; std::vector<size_t> off;
  std::vector<const char*> view;                                 // per read: where the sequence lies in a mapped query file, or nullptr (then arena + off)
  bool nt16 = false; std::vector<uint8_t> rev;                   // a batch of a BAM file: the arena holds 4-bit codes (mm_seqset_add_nt16), rev per read
  // --base-qualities (keep_q: the batch was read under the flag; the two vectors stay empty otherwise): per read where its quality bytes lie in a mapped
  // query file, or their offset in the arena, or neither (NO_QUAL: a FASTA record, a BAM record without); qual_offset: 33 for text, 0 for a BAM's Phred bytes
  static constexpr size_t NO_QUAL = (size_t)-1;
  bool keep_q = false; int qual_offset = 33;
  std::vector<const char*> qview; std::vector<size_t> qoff;
  // --mods (keep_m: the batch was read from a BAM under the flag; the vectors stay empty otherwise): the parsed MM/ML groups of the reads one behind the
  // other, read r's are [mod_goff[r], mod_goff[r + 1]), with mod_has[r] == 0 for a read without tags
  bool keep_m = false;
  std::vector<uint8_t> mod_has; std::vector<size_t> mod_goff{0}; ModGroups mod;
  void put_mods(const ModGroups* g) {                            // the read added last (g == nullptr: it has no groups)
    keep_m = true; mod_has.push_back(g ? 1 : 0);
    if (g) {
      const int64_t k0 = mod.off.back();
      mod.base.insert(mod.base.end(), g->base.begin(), g->base.end()); mod.code.insert(mod.code.end(), g->code.begin(), g->code.end()); mod.mode.insert(mod.mode.end(), g->mode.begin(), g->mode.end());
      for (size_t i = 1; i < g->off.size(); ++i) mod.off.push_back(k0 + g->off[i]);
      mod.skips.insert(mod.skips.end(), g->skips.begin(), g->skips.end()); mod.ml.insert(mod.ml.end(), g->ml.begin(), g->ml.end());
    }
    mod_goff.push_back(mod.base.size());
  }
  int add_mods_to(mm_seqset* s, size_t r) const {                 // mm_seqset_add_mods for read r, which was added to s last (MM_OK where it has no groups)
    if (!keep_m || !mod_has[r]) return MM_OK;
    const size_t g0 = mod_goff[r];
    return mm_seqset_add_mods(s, (int32_t)(mod_goff[r + 1] - g0), mod.base.data() + g0, mod.code.data() + g0, mod.mode.data() + g0, mod.off.data() + g0, mod.skips.data(), mod.ml.data());
  }
  char* arena = nullptr; size_t cap = 0, used = 0;
  size_t seq = 0, file = 0;
  ~Batch() { free(arena); }
  void reserve(size_t want) {
    if (want <= cap) return;
    const size_t HP = (size_t)2 << 20, ncap = (std::max(want, cap + cap / 2) + HP - 1) / HP * HP;
    char* na = (char*)aligned_alloc(HP, ncap);
    if (!na) die("out of host memory for the read batch");
    madvise(na, ncap, MADV_HUGEPAGE);
    if (used) memcpy(na, arena, used);
    free(arena); arena = na; cap = ncap;
  }
  void put(const std::string& q) { reserve(used + q.size() + 1); memcpy(arena + used, q.data(), q.size()); off.push_back(used); view.push_back(nullptr); used += q.size(); }
  void put_view(const char* p) { off.push_back(0); view.push_back(p); }
  const char* seq_of(size_t r) const { return view[r] ? view[r] : arena + off[r]; }
  const char* qual_of(size_t r) const { return !keep_q ? nullptr : qview[r] ? qview[r] : qoff[r] != NO_QUAL ? arena + qoff[r] : nullptr; }   // nullptr: read r has no qualities
  void put_qual(const char* p, size_t n, bool reversed = false) {   // read r's n quality bytes into the arena (p == nullptr: it has none)
    qview.push_back(nullptr);
    if (!p) { qoff.push_back(NO_QUAL); return; }
    reserve(used + n + 1);
    if (reversed) std::reverse_copy(p, p + n, arena + used); else memcpy(arena + used, p, n);
    qoff.push_back(used); used += n;
  }
  void add(SeqFile& f) {                                         // the record `f` just returned
    names.push_back(f.name); lens.push_back((int)f.length());
    if (f.view) put_view(f.view); else put(f.seq);
    if (f.keep_qual) {
      keep_q = true;
      if (f.qview) { qview.push_back(f.qview); qoff.push_back(NO_QUAL); }
      else put_qual(f.has_qual ? f.qual.data() : nullptr, f.qual.size());
    }
  }
  // a BAM record's codes as they are, or (MM_BAM_HOST_DECODE) decoded to ASCII here; keep: its qualities behind them (turned back with the bases where the
  // host decodes, by the library's kernel otherwise)
  void put_nt16(const bam::Record& r, bool keep) {
    const size_t nb = nt16 ? ((size_t)r.l_seq + 1) / 2 : (size_t)r.l_seq;
    reserve(used + nb + 1);
    if (nt16) { memcpy(arena + used, r.seq, nb); rev.push_back(r.reverse() ? 1 : 0); }
    else bam::nt16_to_ascii(r.seq, (size_t)r.l_seq, r.reverse(), arena + used);
    names.push_back(r.name); lens.push_back((int)r.l_seq); off.push_back(used); view.push_back(nullptr); used += nb;
    if (keep) { keep_q = true; qual_offset = 0; put_qual((const char*)r.qual, (size_t)r.l_seq, !nt16 && r.reverse()); }
  }
  void reset() {
    names.clear(); lens.clear(); off.clear(); view.clear(); rev.clear(); qview.clear(); qoff.clear(); nt16 = false; keep_q = false; qual_offset = 33; used = 0;
    keep_m = false; mod_has.clear(); mod_goff.assign(1, 0); mod.clear();
  }
  int64_t bases() const { int64_t b = 0; for (int L : lens) b += L; return b; }
  void absorb(Batch& o) {                                        // o's reads behind this batch's (the block parser's small batches joined up to the batch limits)
    const size_t base = used;
    if (o.used) { reserve(used + o.used); memcpy(arena + used, o.arena, o.used); used += o.used; }
    for (size_t i = 0; i < o.names.size(); ++i) { names.push_back(std::move(o.names[i])); lens.push_back(o.lens[i]); view.push_back(o.view[i]); off.push_back(o.view[i] ? 0 : base + o.off[i]); }
    if (o.keep_q) {
      keep_q = true;
      for (size_t i = 0; i < o.qoff.size(); ++i) { qview.push_back(o.qview[i]); qoff.push_back(o.qoff[i] == NO_QUAL ? NO_QUAL : base + o.qoff[i]); }
    }
  }
};

// a reader thread parses the query files into batches (bounded queue); `take` hands them out in order, nullptr at the end
struct Reader {
  std::mutex m; std::condition_variable cv; std::deque<std::unique_ptr<Batch>> queue, spare; bool done = false, started = false; size_t max_queued = 2;
  std::vector<size_t> file_end;                                // file_end[f] = number of batches of files 0..f (set when file f has been read to its end)
  std::thread th;
  std::unique_ptr<Batch> take() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return !queue.empty() || done; });
    if (queue.empty()) return nullptr;
    auto b = std::move(queue.front()); queue.pop_front();
    cv.notify_all();
    return b;
  }
  void recycle(std::unique_ptr<Batch> b) { b->reset(); std::lock_guard<std::mutex> lk(m); spare.push_back(std::move(b)); }
  ~Reader() { if (th.joinable()) th.join(); }
};

// The reader thread's work.  It is given what it needs and nothing else of the run: the queue it fills, the query files, the batch limits, the device its
// inflate context lives on, the run's phase clock, the mapped query files (alive until the end of the run: the batches point into them), the switches.
struct QueryReader {
  Reader& reader; const std::vector<std::string>& queries; const int64_t BATCH_READS, BATCH_BASES; const int dev0; PhaseClock& pc; std::deque<MappedFile>& mapped; const CliSwitches& sw;
  const bool keep_qual;                                          // --base-qualities: the batches carry the reads' qualities
  const ModsOpts* const mods;                                    // --mods (null without): the batches of a BAM file carry the reads' parsed MM/ML groups
  ModGroups mod_groups; ModCounters mod_n;                       // the record at hand; the counters of the current query file
  size_t q_reads = 0, q_with = 0;                                // under the flag: the reads of the current query file, and those of them with qualities
  using Emit = std::function<void(std::unique_ptr<Batch>)>;
  size_t seq = 0;
  double r_waited = 0;                                           // the reader's own rate (MM_CLI_TIMING): its wall time without what it waited for a free queue slot
  // bgzip text is inflated on the device a segment at a time (mm_bgzf_inflate), on a context of the reader's own on the first device;
  // MM_BGZF_HOST_INFLATE=1: through zlib's sequential gz reader instead.  BAM stays on the host's TaskPool unless MM_BAM_DEVICE_INFLATE=1:
  // on 16 CPUs the kernel (1.7 GB/s on BAM) is slower than zlib on 8 threads, though it takes a third of the host CPU.
  mm_ctx* zctx = nullptr;
  std::vector<int64_t> z_coff, z_ooff; std::vector<int32_t> z_clen, z_st;
  bam::SegmentInflater device_inflate;

  QueryReader(Reader& reader_, const std::vector<std::string>& queries_, int64_t batch_reads, int64_t batch_bases, int dev0_, PhaseClock& pc_, std::deque<MappedFile>& mapped_, const CliSwitches& sw_,
              bool keep_qual_ = false, const ModsOpts* mods_ = nullptr)
      : reader(reader_), queries(queries_), BATCH_READS(batch_reads), BATCH_BASES(batch_bases), dev0(dev0_), pc(pc_), mapped(mapped_), sw(sw_), keep_qual(keep_qual_), mods(mods_) {
    if (!sw.bgzf_host_inflate) device_inflate = [this](const uint8_t* file, const bam::SegBlock* b, size_t n, uint8_t* dst) { inflate_segment(file, b, n, dst); };
  }
  ~QueryReader() { if (zctx) mm_ctx_destroy(zctx); }
  QueryReader(const QueryReader&) = delete;

  void need_zctx() { if (!zctx && mm_ctx_create(dev0, &zctx) != MM_OK) die("cannot create the reader's inflate context"); }
  void inflate_segment(const uint8_t* file, const bam::SegBlock* b, size_t n, uint8_t* dst) {
    need_zctx();
    z_coff.resize(n); z_clen.resize(n); z_ooff.resize(n); z_st.assign(n, 0);
    for (size_t i = 0; i < n; ++i) { z_coff[i] = (int64_t)(b[i].off - b[0].off); z_clen[i] = (int32_t)b[i].bs; z_ooff[i] = (int64_t)(b[i].out - b[0].out); }
    const int64_t comp = (int64_t)(b[n - 1].off + b[n - 1].bs - b[0].off), out = (int64_t)(b[n - 1].out + b[n - 1].isize - b[0].out);
    const int rc = mm_bgzf_inflate(zctx, file + b[0].off, comp, z_coff.data(), z_clen.data(), (int32_t)n, dst + b[0].out, out, z_ooff.data(), z_st.data());
    if (rc == MM_ERR_DATA) for (size_t i = 0; i < n; ++i) if (z_st[i] != 0) throw bam::Error(bam::bgzf_status_message(z_st[i], b[i].off));
    if (rc != MM_OK) die(std::string("device inflate failed: ") + mm_last_error(zctx));
  }
  std::unique_ptr<Batch> fresh() {
    std::unique_ptr<Batch> b;
    { std::lock_guard<std::mutex> lk(reader.m); if (!reader.spare.empty()) { b = std::move(reader.spare.back()); reader.spare.pop_back(); } }
    if (!b) b = std::make_unique<Batch>();
    return b;
  }
  void enqueue(std::unique_ptr<Batch> b, size_t fi) {
    b->seq = seq++; b->file = fi;
    if (keep_qual) { q_reads += b->names.size(); for (size_t r = 0; r < b->names.size(); ++r) q_with += b->qual_of(r) != nullptr; }
    if (sw.timing) std::cerr << "INFO, reader: batch of " << b->names.size() << " reads parsed at +" << std::chrono::duration<double>(std::chrono::steady_clock::now() - pc.t0).count() << " s\n";
    std::unique_lock<std::mutex> lk(reader.m);
    const auto w0 = std::chrono::steady_clock::now();
    reader.cv.wait(lk, [&] { return reader.queue.size() < reader.max_queued; });
    r_waited += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    reader.queue.push_back(std::move(b));
    reader.cv.notify_all();
  }
  size_t first_reserve(int64_t len) const { return (size_t)std::min<int64_t>(BATCH_BASES, len * BATCH_READS) + ((size_t)64 << 20); }   // the arena of a batch of records like its first
  // records -> batches filled up to the batch limits, handed to `emit`: next() steps to the next record (false: there is none), length() is its length,
  // add(batch) puts it into the batch
  template <typename Next, typename Len, typename Add> void fill_batches(Next&& next, Len&& length, Add&& add, const Emit& emit) {
    bool more = true;
    while (more) {
      std::unique_ptr<Batch> b = fresh();
      int64_t bases = 0;
      while ((int64_t)b->names.size() < BATCH_READS && bases < BATCH_BASES) {
        if (!(more = next())) break;
        bases += length();
        add(*b);
      }
      if (b->names.empty()) { std::lock_guard<std::mutex> lk(reader.m); reader.spare.push_back(std::move(b)); break; }
      emit(std::move(b));
    }
  }
  // records of `f` while they start before `stop` (memory mode; (size_t)-1: all) -> batches handed to `emit`; false if the reader
  // gave up on the file (a truncated quality string ends the file for kseq, kseq.h:204)
  bool parse_into(SeqFile& f, size_t stop, const Emit& emit) {
    bool gave_up = false;
    fill_batches([&] {
                   if (stop != (size_t)-1) { const size_t ps = f.peek_start(); if (ps == (size_t)-1 || ps >= stop) return false; }
                   if (!f.next()) { gave_up = stop != (size_t)-1; return false; }
                   return true;
                 },
                 [&] { return (int64_t)f.length(); },
                 [&](Batch& b) { if (b.names.empty() && !f.view) b.reserve(first_reserve((int64_t)f.length())); b.add(f); }, emit);
    return !gave_up;
  }
  void parse_all(SeqFile& f, size_t fi) { parse_into(f, (size_t)-1, [&](std::unique_ptr<Batch> b) { enqueue(std::move(b), fi); }); }

  void read_bam(size_t fi) {                                     // records -> batches of 4-bit codes, packed on the device
    const unsigned P = (unsigned)std::max<unsigned>(1, std::min<unsigned>(32, mm::cpu_budget() / 2));
    try {
      bam::Reader br(queries[fi], P, (1LL << 29) - 1, true, sw.bam_device_inflate ? device_inflate : nullptr, mods != nullptr);
      bam::Record r;
      auto put_mods = [&](Batch& b) {                              // --mods: the record's MM/ML groups, which speak of the read as sequenced, behind its bases
        try {
          const bool has = mods_parse(*mods, r.mm, r.ml, r.mn, r.l_seq, mod_groups, mod_n);
          ++mod_n.reads; mod_n.with_tags += has;
          b.put_mods(has ? &mod_groups : nullptr);
        } catch (const ModTagError& e) { die("Error reading BAM: " + queries[fi] + ": read " + r.name + ": " + e.what()); }
      };
      fill_batches([&] { return br.next(r); }, [&] { return (int64_t)r.l_seq; },
                   [&](Batch& b) {
                     if (b.names.empty()) { b.nt16 = !sw.bam_host_decode; b.reserve(first_reserve((int64_t)r.l_seq)); }
                     b.put_nt16(r, keep_qual);
                     if (mods) put_mods(b);
                   },
                   [&](std::unique_ptr<Batch> b) { enqueue(std::move(b), fi); });
    } catch (const bam::Error& e) { die(std::string("Error reading BAM: ") + e.what()); }
  }
  void read_bgzf_text(size_t fi) {                               // bgzip FASTA/FASTQ: the sequential record parse over device-inflated segments
    try {
      bam::BgzfStream z(queries[fi], 1, device_inflate, false);
      SeqFile f([&](std::vector<unsigned char>& buf) -> size_t {
        while (!z.at_end()) if (const size_t n = z.inflate_segment(buf, 0)) return n;
        return 0;
      });
      f.keep_qual = keep_qual;
      parse_all(f, fi);
    } catch (const bam::Error& e) { die(std::string("Error reading ") + queries[fi] + ": " + e.what()); }
  }
  void read_gzip_text(size_t fi) {                               // plain gzip FASTA/FASTQ: the sequential record parse over device-inflated pieces
    need_zctx();
    {
      DeviceGzip z(zctx, queries[fi]);
      SeqFile f([&](std::vector<unsigned char>& buf) -> size_t { return z.fill(buf); });
      f.keep_qual = keep_qual;
      parse_all(f, fi);
    }
    (void)mm_ctx_release_cached(zctx);                           // (the stream's slots, up to 4.5 GiB, back to the driver beside the mapping)
  }
  void read_sequential(size_t fi) { SeqFile f(queries[fi]); f.keep_qual = keep_qual; parse_all(f, fi); }   // gzip through zlib, pipes, ...
  void read_blocks(MappedFile& mf, size_t fi) {
    // blocks of the mapped file, parsed by several threads, handed on in file order; a block's batches only go out once the
    // block before it has been seen to end exactly where this one starts
    const size_t blk = sw.block_bytes;
    const size_t nb = std::max<size_t>(1, (mf.size + blk - 1) / blk);
    std::vector<size_t> start(nb + 1, mf.size);
    start[0] = 0;
    struct Block { std::vector<std::unique_ptr<Batch>> out; size_t next = 0; bool done = false, empty = false, over = false; };   // next: first record start behind the block's records
    std::vector<Block> blocks(nb);
    std::mutex bm; std::condition_variable bcv; size_t next_block = 0, consumed = 0; bool abandon = false;
    const unsigned P = (unsigned)std::max<size_t>(1, std::min<size_t>({nb, (size_t)8, (size_t)std::max(1u, mm::cpu_budget() / 2)}));
    auto worker = [&]() {
      for (;;) {
        size_t j;
        {
          std::unique_lock<std::mutex> lk(bm);
          bcv.wait(lk, [&] { return abandon || next_block >= nb || next_block < consumed + P + 2; });   // not too far ahead of the consumer
          if (abandon || next_block >= nb) return;
          j = next_block++;
        }
        const auto b_t0 = std::chrono::steady_clock::now();
        if (j > 0) start[j] = mf.sync(j * blk, std::min(mf.size, (j + 1) * blk));   // (only this thread writes start[j]; read after `done`)
        Block& B = blocks[j];
        const size_t lim = std::min(mf.size, (j + 1) * blk);
        if (j == 0 || start[j] < lim) {                        // records that start in [start[j], lim)
          SeqFile f(mf.data, j == 0 ? 0 : start[j], mf.size);
          f.keep_qual = keep_qual;
          B.over = !parse_into(f, lim, [&](std::unique_ptr<Batch> b) { B.out.push_back(std::move(b)); });
          B.next = f.peek_start();
        } else B.empty = true;                                 // no record start was recognised in this block
        pc.add("R parse threads busy (summed over the block parser's threads)", std::chrono::duration<double>(std::chrono::steady_clock::now() - b_t0).count());
        { std::lock_guard<std::mutex> lk(bm); B.done = true; }
        bcv.notify_all();
      }
    };
    pc.add("R parse threads", (double)P);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < P; ++t) pool.emplace_back(worker);
    // `expect`: where the parse stands = the start of the first record not handed on yet.  A block continues the parse iff it
    // starts exactly there (block 0 starts at the file's first record by construction).
    size_t expect = 0; bool chain_ok = true, file_over = false;
    std::unique_ptr<Batch> pend; int64_t pend_bases = 0;
    for (size_t j = 0; j < nb && chain_ok && !file_over; ++j) {
      { std::unique_lock<std::mutex> lk(bm); bcv.wait(lk, [&] { return blocks[j].done; }); }
      Block& B = blocks[j];
      if (!B.empty) {
        if (j > 0 && start[j] != expect) { chain_ok = false; break; }
        for (auto& b : B.out) {                                 // a block ends where its 128 MB end, not where a batch is full: its last batch goes on in the next block
          if (pend && ((int64_t)(pend->names.size() + b->names.size()) > BATCH_READS || pend_bases + b->bases() > BATCH_BASES)) { enqueue(std::move(pend), fi); pend_bases = 0; }
          if (!pend) { pend_bases = b->bases(); pend = std::move(b); }
          else { pend_bases += b->bases(); pend->absorb(*b); reader.recycle(std::move(b)); }
        }
        B.out.clear();
        if (B.over || B.next == (size_t)-1) { file_over = true; break; }
        expect = B.next;
      } else if (expect < std::min(mf.size, (j + 1) * blk)) { chain_ok = false; break; }   // a record starts in this block, but none was recognised
      { std::lock_guard<std::mutex> lk(bm); consumed = j + 1; } bcv.notify_all();
    }
    { std::lock_guard<std::mutex> lk(bm); abandon = true; } bcv.notify_all();
    for (auto& t : pool) t.join();
    if (pend) enqueue(std::move(pend), fi);
    if (!chain_ok) {                                           // a block did not start where the parse stood: the rest sequentially, from there
      for (auto& B : blocks) for (auto& b : B.out) reader.recycle(std::move(b));
      SeqFile f(mf.data, expect, mf.size);
      f.keep_qual = keep_qual;
      parse_into(f, (size_t)-1, [&](std::unique_ptr<Batch> b) { enqueue(std::move(b), fi); });
    }
  }

  void mods_info(const std::string& q, bool is_bam) {            // --mods: one line per query file, with the reason where its bedMethyl file will be empty
    if (!is_bam) std::cout << "INFO, --mods: " << q << " is not a BAM file and carries no MM/ML tags: its bedMethyl file is empty\n";
    else
      std::cout << "INFO, --mods: " << q << ": " << mod_n.reads << " reads, " << mod_n.with_tags << " with MM/ML tags" << (mod_n.with_tags ? "" : ": its bedMethyl file is empty") << "; dropped: "
                << mod_n.minus_groups << " groups of strand -, " << mod_n.n_groups << " groups of base N, " << mod_n.mn_mismatch << " reads whose MN differs from their length\n";
    mod_n = ModCounters{};
  }
  // every query file in turn, by the kind its content shows; the lap of the kinds that have one, and the end of the file for the writer
  void run() {
    const auto r_t0 = std::chrono::steady_clock::now();
    for (size_t fi = 0; fi < queries.size(); ++fi) {
      const std::string& q = queries[fi];
      const bool is_bam = bam::is_bam_file(q), is_bgzf = !is_bam && !sw.bgzf_host_inflate && bam::is_bgzf_file(q);
      const bool is_gzip = !is_bam && !is_bgzf && !sw.gzip_host_inflate && is_plain_gzip_file(q);
      const auto f_t0 = std::chrono::steady_clock::now();
      const char* lap = nullptr;
      if (is_bam) { read_bam(fi); lap = "R BAM reader (inflate + parse, without waiting for a queue slot)"; }
      else if (is_bgzf) { read_bgzf_text(fi); lap = "R bgzip reader (inflate + parse, without waiting for a queue slot)"; }
      else if (is_gzip) { read_gzip_text(fi); lap = "R gzip reader (device inflate + parse, without waiting for a queue slot)"; }
      else {
        mapped.emplace_back();
        if (sw.no_mmap || !mapped.back().open(q)) { mapped.pop_back(); read_sequential(fi); }
        else read_blocks(mapped.back(), fi);
      }
      if (lap) pc.add(lap, std::chrono::duration<double>(std::chrono::steady_clock::now() - f_t0).count());
      if (keep_qual && q_reads && !q_with) std::cout << "INFO, --base-qualities: " << q << " carries no qualities: every base of its reads is without one (0xFF in PREFIX.bam)\n";
      q_reads = q_with = 0;
      if (mods) mods_info(q, is_bam);
      std::lock_guard<std::mutex> lk(reader.m); reader.file_end.push_back(seq); reader.cv.notify_all();
    }
    { const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - r_t0).count();
      pc.add("R reader thread wall time without waiting for a queue slot", wall - r_waited); pc.add("R reader waited for a queue slot", r_waited); }
    std::lock_guard<std::mutex> lk(reader.m); reader.done = true; reader.cv.notify_all();
  }
};

}  // namespace
