// mapDirectly --bam-sorted (implies --edit-distance; not in the reference): PREFIX.sorted.bam, the records of PREFIX.bam in ascending (refID, pos, place in
// PREFIX.bam), and PREFIX.sorted.bam.bai ("Sorted BAM"; the index's canonical form: include/metamaps_hip.h, mm_bam_sorter_*).
//   batch     the context that mapped a batch encodes its records once more as one sorted run (mm_bam_encode_sorted) and keeps the run's keys: per record
//             refID, pos, end = pos + max(1, reference span) and the offset in the run's inflated bytes (SortedRun).
//   writer    the runs' members go to PREFIX.sorted.bam.tmp in batch order, the keys stay in host memory (SortedFile): 20 bytes per record.
//   merge     after the run's last batch, on the first device, per query file: the temp file is mapped, mm_bam_sorter_* merges the runs a window at a
//             time (MM_BAM_SORT_WINDOW_MB), the header (bam_header, sorted), the windows' members and the end-of-file block are written, then the index; the
//             temp file goes.  Runs are added in batch order and a run is in job order among equal keys, so the order is a stable sort of PREFIX.bam and the
//             files do not depend on the batch size, the devices or the window.
// Not provided: CSI (a contig of 2^29 bases or more is refused), unmapped records, name sort, merging across query files, samtools-identical index bytes.
#pragma once
#include "bam_out.hpp"
#include "cli_device.hpp"
#include "paf_out.hpp"
#include "side_files.hpp"
#include <deque>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

// one batch's sorted run: its members and its records' keys in the run's order
struct SortedRun { std::string members; std::vector<int64_t> raw_off; std::vector<int32_t> ref, pos, end; };

// the batch's records as a sorted run, encoded on the context that mapped it
void sorted_run_encode(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const BamFields& F, const BatchAlignment& al, int64_t n_jobs, SortedRun& run) {
  mm_bam* b = nullptr;
  ck(ctx, mm_bam_encode_sorted(ctx, reads, reference, n_jobs, F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(), al.op_off.data(), al.ops.data(),
                               F.flag.data(), F.mapq.data(), F.name_off.data(), F.all_names.data(), 0, &b), "sorted BAM records");
  int64_t n = 0, raw = 0, bytes = 0;
  mm_bam_sizes(b, &n, &raw, &bytes);
  std::vector<int64_t> job((size_t)n);
  run.members.resize((size_t)bytes); run.raw_off.resize((size_t)n + 1);
  if (bytes) mm_bam_fetch(b, (uint8_t*)&run.members[0]);
  mm_bam_fetch_records(b, job.data(), run.raw_off.data());
  mm_bam_destroy(b);
  run.ref.resize((size_t)n); run.pos.resize((size_t)n); run.end.resize((size_t)n);
  for (size_t i = 0; i < (size_t)n; ++i) {
    const size_t j = (size_t)job[i];
    run.ref[i] = F.contig[j]; run.pos[i] = (int32_t)al.first[j]; run.end[i] = (int32_t)std::max(al.first[j] + 1, al.last[j] + 1);
  }
}

// a query file's runs: the members in PREFIX.sorted.bam.tmp, the keys here
struct SortedFile {
  struct Run { int64_t at, bytes; size_t rec0, n; };
  std::string tmp; FILE* f = nullptr; int64_t bytes = 0;
  std::vector<Run> runs; std::vector<int64_t> raw_off; std::vector<int32_t> ref, pos, end;   // (raw_off: n + 1 entries per run, back to back)
  void append(const std::string& prefix, SortedRun& r) {          // (the temp file comes with the first run that has a record)
    if (r.ref.empty()) return;
    if (!f) {
      tmp = prefix + ".sorted.bam.tmp";
      f = fopen(tmp.c_str(), "wb");
      if (!f) die("Cannot open output file " + tmp);
    }
    if (fwrite(r.members.data(), 1, r.members.size(), f) != r.members.size()) die("Error writing " + tmp);
    runs.push_back(Run{bytes, (int64_t)r.members.size(), ref.size(), r.ref.size()});
    bytes += (int64_t)r.members.size();
    raw_off.insert(raw_off.end(), r.raw_off.begin(), r.raw_off.end());
    ref.insert(ref.end(), r.ref.begin(), r.ref.end()); pos.insert(pos.end(), r.pos.begin(), r.pos.end()); end.insert(end.end(), r.end.begin(), r.end.end());
    r = SortedRun();
  }
  void close() { if (f && fclose(f) != 0) die("Error writing " + tmp); f = nullptr; }
};

// BAI holds coordinates below 2^29
void sorted_bam_check_contigs(const std::vector<std::string>& cname, const std::vector<int>& clen) {
  for (size_t c = 0; c < clen.size(); ++c)
    if ((int64_t)clen[c] >= ((int64_t)1 << 29)) die("--bam-sorted: contig " + cname[c] + " has 2^29 bases or more, which a BAI index cannot hold (CSI is not provided)");
}

// what mm_bam_sorter_fetch gives after a window or the index, appended to a file
void sorter_product_to(mm_bam_sorter* s, int64_t bytes, std::vector<uint8_t>& buf, FILE* out, const std::string& name) {
  buf.resize((size_t)std::max<int64_t>(bytes, 1));
  mm_bam_sorter_fetch(s, buf.data());
  if (fwrite(buf.data(), 1, (size_t)bytes, out) != (size_t)bytes) die("Error writing " + name);
}

// the merge of a query file's runs on `ctx`: PREFIX.sorted.bam and PREFIX.sorted.bam.bai; the temp file goes.  head: the sorted header's members
void sorted_bam_write(mm_ctx* ctx, SortedFile& sf, const std::string& prefix, const std::string& head, const std::vector<int>& clen, int64_t window_bytes) {
  const std::string bam = prefix + ".sorted.bam", bai = bam + ".bai";
  sf.close();
  void* map = MAP_FAILED; int fd = -1;
  if (sf.bytes > 0) {
    fd = ::open(sf.tmp.c_str(), O_RDONLY);
    if (fd >= 0) map = mmap(nullptr, (size_t)sf.bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) die("Cannot map " + sf.tmp);
  }
  mm_bam_sorter* s = nullptr;
  const std::vector<int32_t> len(clen.begin(), clen.end());
  ck(ctx, mm_bam_sorter_create(ctx, (int32_t)len.size(), len.data(), window_bytes, &s), "sorter");
  size_t off_at = 0;
  for (const SortedFile::Run& r : sf.runs) {
    ck(ctx, mm_bam_sorter_add_run(s, (const uint8_t*)map + r.at, r.bytes, (int64_t)r.n, sf.raw_off.data() + off_at, sf.ref.data() + r.rec0, sf.pos.data() + r.rec0, sf.end.data() + r.rec0),
       "sorted run");
    off_at += r.n + 1;
  }
  int64_t n_windows = 0, stream = 0, bytes = 0;
  ck(ctx, mm_bam_sorter_plan(s, &n_windows, &stream), "sort plan");
  FILE* out = fopen(bam.c_str(), "wb");
  if (!out || fwrite(head.data(), 1, head.size(), out) != head.size()) die("Error writing " + bam);
  std::vector<uint8_t> buf;
  for (int64_t w = 0; w < n_windows; ++w) {
    ck(ctx, mm_bam_sorter_window(s, w, &bytes), "sorted window");
    sorter_product_to(s, bytes, buf, out, bam);
  }
  if (fwrite(kBgzfEof, 1, sizeof kBgzfEof, out) != sizeof kBgzfEof || fclose(out) != 0) die("Error writing " + bam);
  ck(ctx, mm_bam_sorter_index(s, (int64_t)head.size(), &bytes), "BAM index");
  FILE* idx = fopen(bai.c_str(), "wb");
  if (!idx) die("Error writing " + bai);
  sorter_product_to(s, bytes, buf, idx, bai);
  if (fclose(idx) != 0) die("Error writing " + bai);
  mm_bam_sorter_destroy(s);
  if (map != MAP_FAILED) munmap(map, (size_t)sf.bytes);
  if (fd >= 0) ::close(fd);
  if (!sf.tmp.empty()) ::unlink(sf.tmp.c_str());
}

}  // namespace
