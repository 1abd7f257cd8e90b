// The reference FASTA of mapDirectly / index (winSketch.hpp:180-365): parsed, packed and uploaded to every device that builds indexes from it.
// Two sources feed one consumer: a plain file mapped into memory and parsed in blocks by several threads, or a stream (plain gzip inflated on the
// device, or whatever the sequential reader opens) parsed by one thread two groups ahead.
#pragma once
#include "../cpu_budget.hpp"
#include "cli_device.hpp"
#include "cli_switches.hpp"
#include "query_reader.hpp"

namespace {

struct ReferenceLoader {
  struct Group { std::deque<std::string> seq; std::vector<std::string> names; uint64_t bases = 0; };
  using Emit = std::function<void(std::unique_ptr<Group>)>;

  const CliSwitches& sw;
  const std::vector<Dev>& devs;
  PhaseClock& pc;
  std::vector<std::string>& cname; std::vector<int>& clen; uint64_t& ref_bases;   // the run's contig table, in file order
  std::vector<std::vector<mm_seqset*>> parts;                    // per device: the uploaded groups, joined by concat()
  double t_pack = 0;

  ReferenceLoader(const CliSwitches& sw_, const std::vector<Dev>& devs_, size_t n_devices, PhaseClock& pc_, std::vector<std::string>& cname_,
                  std::vector<int>& clen_, uint64_t& ref_bases_)
      : sw(sw_), devs(devs_), pc(pc_), cname(cname_), clen(clen_), ref_bases(ref_bases_), parts(n_devices) {}

  void consume(Group& g) {                                         // names and lengths in file order, then pack + upload to every device
    for (size_t i = 0; i < g.seq.size(); ++i) { cname.push_back(std::move(g.names[i])); clen.push_back((int)g.seq[i].size()); ref_bases += g.seq[i].size(); }
    const auto t0 = std::chrono::steady_clock::now();
    on_each(parts.size(), [&](size_t d) {
      mm_seqset* p; ck(devs[d].ctx, mm_seqset_create(devs[d].ctx, &p), "seqset");
      for (auto& q : g.seq) ck(devs[d].ctx, mm_seqset_add_view(p, q.data(), (int64_t)q.size()), "add contig");
      ck(devs[d].ctx, mm_seqset_upload(p), "upload reference");
      parts[d].push_back(p);
    });
    t_pack += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  // records of `f` (all, or those that start before `stop` in memory mode) in groups of GROUP_BASES handed to `emit`; false when the
  // reader gave up before `stop` (a truncated quality string ends the file for kseq, kseq.h:204)
  bool parse_groups(SeqFile& f, size_t stop, const Emit& emit) const {
    const uint64_t GROUP_BASES = sw.ref_group_bases;
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
  }

  // A plain file: blocks of the mapping parsed by several threads (the block parser of the query files, query_reader.hpp: a block's records
  // count only once the block before it has been seen to end exactly where this one starts), consumed — packed, uploaded — in file
  // order.  The winSketch.hpp:242-252 loop reads contig by contig; here the text of at most P + 2 blocks of 256 MB is resident, and the
  // mapped pages of a block are given back once it is consumed (they would count as resident until the end otherwise: 27 GB).
  void load_mapped(MappedFile& rmf) {
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
    if (!chain_ok) {                                             // a block did not start where the parse stood: the rest sequentially, from there
      for (auto& B : blocks) B.out.clear();
      SeqFile f(rmf.data, expect, rmf.size);
      parse_groups(f, (size_t)-1, [&](std::unique_ptr<Group> g) { consume(*g); });
    }
  }

  // gzip, pipes: a parser thread fills groups, the calling thread packs and uploads each while the next one is parsed.  Host memory: two groups.
  void load_streamed(const std::string& ref) {
    std::mutex gm; std::condition_variable gcv; std::deque<std::unique_ptr<Group>> ready; bool parsed = false;
    double t_gzip = -1;                                          // the device gzip reader's wall time (its phase line), -1 if zlib read the file
    const Emit push = [&](std::unique_ptr<Group> g) {            // (whichever source parses: at most two groups wait for the consumer)
      std::unique_lock<std::mutex> lk(gm); gcv.wait(lk, [&] { return ready.size() < 2; }); ready.push_back(std::move(g)); gcv.notify_all();
    };
    std::thread parser([&]() {
      if (!sw.gzip_host_inflate && is_plain_gzip_file(ref)) {     // plain gzip: inflated on the device, on a context of the parser's own
        const auto g_t0 = std::chrono::steady_clock::now();
        mm_ctx* gctx = nullptr;
        if (mm_ctx_create(devs[0].phys, &gctx) != MM_OK) die("cannot create the reference reader's inflate context");
        {
          DeviceGzip z(gctx, ref);
          SeqFile f([&](std::vector<unsigned char>& buf) -> size_t { return z.fill(buf); });
          parse_groups(f, (size_t)-1, push);
        }
        mm_ctx_destroy(gctx);
        std::lock_guard<std::mutex> lk(gm); parsed = true; gcv.notify_all();
        t_gzip = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
        return;
      }
      SeqFile f(ref);
      parse_groups(f, (size_t)-1, push);
      std::lock_guard<std::mutex> lk(gm); parsed = true; gcv.notify_all();
    });
    for (;;) {
      std::unique_ptr<Group> g;
      {
        std::unique_lock<std::mutex> lk(gm);
        gcv.wait(lk, [&] { return !ready.empty() || parsed; });
        if (ready.empty()) break;
        g = std::move(ready.front()); ready.pop_front(); gcv.notify_all();
      }
      consume(*g);
    }
    parser.join();
    if (t_gzip >= 0) pc.add("1g reference gzip reader (device inflate + parse, inside 1)", t_gzip);
  }

  // the reference file `ref` into refset[d] of every device
  void load(const std::string& ref, std::vector<mm_seqset*>& refset) {
    MappedFile rmf;
    if (!sw.no_mmap && !sw.ref_sequential && rmf.open(ref)) load_mapped(rmf);
    else load_streamed(ref);
    concat(refset);
  }

  // every device's groups joined into its one reference set
  void concat(std::vector<mm_seqset*>& refset) {
    on_each(parts.size(), [&](size_t d) {
      if (parts[d].size() == 1) { refset[d] = parts[d][0]; return; }
      if (parts[d].empty()) {
        ck(devs[d].ctx, mm_seqset_create(devs[d].ctx, &refset[d]), "seqset");
        ck(devs[d].ctx, mm_seqset_upload(refset[d]), "upload reference");
        return;
      }
      ck(devs[d].ctx, mm_seqset_concat(devs[d].ctx, parts[d].data(), (int)parts[d].size(), &refset[d]), "reference");
      for (auto* p : parts[d]) mm_seqset_destroy(p);
    });
  }
};

}  // namespace
