// Unaligned (or aligned) BAM as a query file for the `metamaps` host program: the BGZF block walk (also of bgzip-compressed FASTA/FASTQ),
// parallel raw inflate of the blocks (or a caller's segment inflater: the CLI's inflates on the device) and the record parse.  Host only, no device
// dependencies: tests/test_bam_reader.cpp checks it on the CPU against a BAM writer in Python.
//
// What a record becomes is what `samtools fastq -n` writes for it: secondary (0x100) and supplementary (0x800) records are skipped, a record
// with 0x10 is the reverse complement of the read as sequenced (the complement of a 4-bit code is its bit reversal: A<->T, C<->G, M<->K, R<->Y,
// V<->B, H<->D; S, W, N and '=' stay), the name is read_name without its NUL, the qualities are handed on as they lie (Record::qual: in the
// record's order, so reversed where 0x10 is set), tags are ignored unless the reader is asked for the base-modification tags (want_tags: the aux fields
// are walked and views of MM, ML and MN handed on), and paired-end flags (0x1, 0x40, 0x80) are NOT interpreted: no /1 or /2 is
// appended.  The bases stay in BAM's packed 4-bit form (two per byte, high nibble first): the
// library packs them on the device (mm_seqset_add_nt16).
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../task_pool.hpp"

namespace bam {

constexpr const char* NT16_ASCII = "=ACMGRSVTWYHKDBN";
inline uint8_t nt16_complement(uint8_t c) { return (uint8_t)(((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3)); }
inline uint8_t nt16_at(const uint8_t* p, size_t i) { return (uint8_t)((p[i >> 1] >> ((i & 1) ? 0 : 4)) & 15); }
// the read as sequenced, in ASCII (what samtools fastq writes; the host-decode cross-check of the CLI)
inline void nt16_to_ascii(const uint8_t* p, size_t n, bool reverse, char* out) {
  if (!reverse) for (size_t i = 0; i < n; ++i) out[i] = NT16_ASCII[nt16_at(p, i)];
  else for (size_t i = 0; i < n; ++i) out[i] = NT16_ASCII[nt16_complement(nt16_at(p, n - 1 - i))];
}

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// BSIZE + 1 of the BGZF block at p (n bytes available), 0 if p is no BGZF block header (a gzip member with the "BC" extra subfield)
inline size_t bgzf_block_size(const uint8_t* p, size_t n) {
  if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
  const size_t xlen = rd16(p + 10);
  if (n < 12 + xlen) return 0;
  for (size_t x = 12; x + 4 <= 12 + xlen;) {
    const size_t slen = rd16(p + x + 2);
    if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) return (size_t)rd16(p + x + 4) + 1;
    x += 4 + slen;
  }
  return 0;
}

// raw inflate of one BGZF block (whole, `bs` bytes at p) into out[isize]; checks ISIZE and CRC32
inline void bgzf_inflate(const uint8_t* p, size_t bs, uint8_t* out, size_t isize, size_t at) {
  const size_t xlen = rd16(p + 10), hdr = 12 + xlen;
  if (bs < hdr + 8) throw Error("corrupt BGZF block at byte " + std::to_string(at));
  z_stream z{};
  if (inflateInit2(&z, -15) != Z_OK) throw Error("zlib inflateInit2 failed");
  z.next_in = const_cast<Bytef*>(p + hdr); z.avail_in = (uInt)(bs - hdr - 8);
  z.next_out = out; z.avail_out = (uInt)isize;
  const int r = inflate(&z, Z_FINISH);
  const size_t got = isize - z.avail_out;
  inflateEnd(&z);
  if (r != Z_STREAM_END || got != isize) throw Error("corrupt BGZF block at byte " + std::to_string(at) + " (inflate failed)");
  if ((uint32_t)crc32(0L, out, (uInt)isize) != rd32(p + bs - 8)) throw Error("corrupt BGZF block at byte " + std::to_string(at) + " (CRC mismatch)");
}

// the message bgzf_inflate throws for a block at file offset `at`, from a block status of a device inflate (mm_bgzf_inflate: 1 deflate
// stream invalid, 2 length != ISIZE — both "inflate failed" for zlib —, 3 CRC32 mismatch, 4 malformed header)
inline std::string bgzf_status_message(int status, size_t at) {
  const std::string m = "corrupt BGZF block at byte " + std::to_string(at);
  return status == 3 ? m + " (CRC mismatch)" : status == 4 ? m : m + " (inflate failed)";
}

// a file that starts with a BGZF block (BAM, or text written by bgzip)
inline bool is_bgzf_file(const std::string& path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  uint8_t b[1024];
  const ssize_t n = pread(fd, b, sizeof b, 0);
  ::close(fd);
  return n >= 18 && bgzf_block_size(b, (size_t)n) >= 26;
}

// a file is BAM if it starts with a BGZF block whose inflated data starts with "BAM\1"; anything else (FASTA, FASTQ, plain gzip) is not
inline bool is_bam_file(const std::string& path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  std::vector<uint8_t> b(65536 + 32);
  const ssize_t n = pread(fd, b.data(), b.size(), 0);
  ::close(fd);
  if (n < 18) return false;
  const size_t bs = bgzf_block_size(b.data(), (size_t)n);
  if (!bs || bs > (size_t)n || bs < 26) return false;
  const size_t isize = rd32(b.data() + bs - 4);
  if (isize < 4 || isize > 65536) return false;
  std::vector<uint8_t> out(isize);
  try { bgzf_inflate(b.data(), bs, out.data(), isize, 0); } catch (const Error&) { return false; }
  return memcmp(out.data(), "BAM\1", 4) == 0;
}

// One aux field: its type (A c C s S i I f Z H B), for B the element type and count, and its value's bytes inside the record (Z, H: without the NUL)
struct AuxField { char tag[2]; char type, sub; const uint8_t* p; size_t bytes, count; };
inline size_t aux_elem_bytes(char t) { return t == 'A' || t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' || t == 'f' ? 4 : 0; }
// the aux fields in [p, end), each handed to fn; false where a field has an unknown type or runs over the end
template <class Fn> bool aux_walk(const uint8_t* p, const uint8_t* end, Fn&& fn) {
  while (p < end) {
    if (end - p < 3) return false;
    AuxField f{{(char)p[0], (char)p[1]}, (char)p[2], 0, p + 3, 0, 1};
    p += 3;
    if (const size_t w = aux_elem_bytes(f.type)) { if ((size_t)(end - p) < w) return false; f.bytes = w; }
    else if (f.type == 'Z' || f.type == 'H') {
      const void* nul = memchr(p, 0, (size_t)(end - p));
      if (!nul) return false;
      f.bytes = (size_t)((const uint8_t*)nul - p); f.count = f.bytes;
      fn(f); p += f.bytes + 1;
      continue;
    } else if (f.type == 'B') {
      if (end - p < 5) return false;
      f.sub = (char)p[0];
      const size_t w = aux_elem_bytes(f.sub), n = rd32(p + 1);
      if (!w || f.sub == 'A' || n > (size_t)(end - p - 5) / w) return false;
      f.p = p + 5; f.count = n; f.bytes = n * w;
      fn(f); p += 5 + f.bytes;
      continue;
    } else return false;
    fn(f); p += f.bytes;
  }
  return true;
}
inline int64_t aux_int(const AuxField& f) {                       // of an integer field (c C s S i I)
  switch (f.type) {
    case 'c': return (int8_t)f.p[0]; case 'C': return f.p[0]; case 's': return (int16_t)rd16(f.p); case 'S': return rd16(f.p);
    case 'i': return (int32_t)rd32(f.p); default: return rd32(f.p);
  }
}

struct Record {
  std::string name;
  const uint8_t* seq = nullptr;   // (l_seq + 1) / 2 bytes of 4-bit codes, valid until the next call of Reader::next
  int64_t l_seq = 0;
  const uint8_t* qual = nullptr;  // l_seq raw Phred bytes in the record's order, valid as long as seq; nullptr: the record has none (its first quality byte is 0xFF)
  uint16_t flag = 0;
  bool reverse() const { return flag & 0x10; }
  // under want_tags: the record's MM, ML and MN fields as they lie (type 0: the record has none), valid as long as seq
  AuxField mm{}, ml{}, mn{};
};

// One block of a segment to inflate: bs bytes at file offset `off`, its isize inflated bytes go to dst + out.
struct SegBlock { size_t off, bs, isize, out; };
// Inflates the n blocks of a segment (consecutive in the file mapped at `file`) into dst, or throws bam::Error with bgzf_inflate's message
// for the first bad block.  With none given, zlib on the host (on a TaskPool); the CLI passes one that inflates on the device.
using SegmentInflater = std::function<void(const uint8_t* file, const SegBlock* blk, size_t n, uint8_t* dst)>;

// The inflated bytes of a memory-mapped BGZF file, a segment (up to SEG_BLOCKS blocks, ~64 MiB of data) at a time.  Without an inflater the
// blocks of a segment are inflated in parallel on a TaskPool of `threads` participants (1: all on the calling thread).  A missing EOF marker
// is a warning on stderr, as in samtools, where `warn_eof` is set.
class BgzfStream {
 public:
  static constexpr size_t SEG_BLOCKS = 1024;
  BgzfStream(const std::string& path, unsigned threads, SegmentInflater inflater = nullptr, bool warn_eof = true)
      : path_(path), inflater_(std::move(inflater)), warn_eof_(warn_eof) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw Error("Cannot open " + path);
    struct stat st;
    if (fstat(fd, &st) != 0) { ::close(fd); throw Error("Cannot stat " + path); }
    size_ = (size_t)st.st_size;
    if (size_) {
      void* p = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd, 0);
      if (p == MAP_FAILED) { ::close(fd); throw Error("Cannot map " + path); }
      madvise(p, size_, MADV_SEQUENTIAL);
      data_ = (const uint8_t*)p;
    }
    ::close(fd);
    if (threads > 1 && !inflater_) pool_ = std::make_unique<TaskPool>(threads - 1);
  }
  ~BgzfStream() { if (data_) munmap((void*)data_, size_); }
  BgzfStream(const BgzfStream&) = delete;
  BgzfStream& operator=(const BgzfStream&) = delete;
  const uint8_t* data() const { return data_; }
  size_t size() const { return size_; }
  bool at_end() const { return foff_ >= size_; }
  size_t blocks() const { return nblocks_; }
  bool eof_marker() const { return eof_seen_; }

  // the next segment's inflated bytes into buf from `at` on (buf grows as needed); returns their number
  size_t inflate_segment(std::vector<uint8_t>& buf, size_t at) {
    std::vector<SegBlock> seg;
    size_t total = 0;
    while (foff_ < size_ && seg.size() < SEG_BLOCKS) {
      const size_t bs = bgzf_block_size(data_ + foff_, size_ - foff_);
      if (!bs) {
        if (size_ - foff_ < 18) throw Error(path_ + ": truncated BGZF block at byte " + std::to_string(foff_));
        throw Error(path_ + ": bad magic: no BGZF block at byte " + std::to_string(foff_));
      }
      if (bs < 26 || foff_ + bs > size_) throw Error(path_ + ": truncated BGZF block at byte " + std::to_string(foff_));
      const size_t isize = rd32(data_ + foff_ + bs - 4);
      if (isize > 65536) throw Error(path_ + ": corrupt BGZF block at byte " + std::to_string(foff_) + " (ISIZE " + std::to_string(isize) + ")");
      seg.push_back(SegBlock{foff_, bs, isize, at + total});
      total += isize;
      foff_ += bs;
      ++nblocks_;
      if (foff_ == size_) {                                      // the last block: BGZF's EOF marker is an empty block of exactly 28 bytes
        eof_seen_ = isize == 0 && bs == 28;
        if (!eof_seen_ && warn_eof_) std::cerr << "[W::bgzf_read_block] EOF marker is absent. The input " << path_ << " is probably truncated" << std::endl;
      }
    }
    if (buf.size() < at + total) buf.resize(at + total + (at + total) / 4);
    if (inflater_) { if (!seg.empty()) inflater_(data_, seg.data(), seg.size(), buf.data()); }
    else {
      auto one = [&](size_t t) { const SegBlock& b = seg[t]; bgzf_inflate(data_ + b.off, b.bs, buf.data() + b.out, b.isize, b.off); };
      if (pool_ && seg.size() > 1) {
        const size_t W = pool_->width();
        pool_->run(W, [&](size_t p) { for (size_t t = p; t < seg.size(); t += W) one(t); });
      } else for (size_t t = 0; t < seg.size(); ++t) one(t);
    }
    if (!seg.empty()) {                                          // the compressed pages of the segment are not needed again
      const uintptr_t a = (uintptr_t)(data_ + seg[0].off) & ~(uintptr_t)4095, b = (uintptr_t)(data_ + foff_) & ~(uintptr_t)4095;
      if (b > a) madvise((void*)a, (size_t)(b - a), MADV_DONTNEED);
    }
    return total;
  }

 private:
  std::string path_;
  SegmentInflater inflater_;
  bool warn_eof_;
  const uint8_t* data_ = nullptr; size_t size_ = 0, foff_ = 0, nblocks_ = 0;
  bool eof_seen_ = false;
  std::unique_ptr<TaskPool> pool_;
};

// Sequential record reader over a BAM: the inflated bytes come a segment at a time from a BgzfStream (`inflater` as there); a record that
// spans two segments is carried over whole.  Errors throw bam::Error with a message; a missing EOF marker is a warning on stderr.
class Reader {
 public:
  static constexpr size_t SEG_BLOCKS = BgzfStream::SEG_BLOCKS;
  Reader(const std::string& path, unsigned threads, int64_t max_len, bool skip_filtered = true, SegmentInflater inflater = nullptr, bool want_tags = false)
      : path_(path), max_len_(max_len), skip_filtered_(skip_filtered), want_tags_(want_tags), z_(path, threads, std::move(inflater)) {
    read_header();
  }
  Reader(const Reader&) = delete;
  Reader& operator=(const Reader&) = delete;

  // the next record (skipping secondary and supplementary ones unless skip_filtered is false); false at the end of the file
  bool next(Record& r) {
    for (;;) {
      if (!need(4)) { if (pos_ != end_) throw Error(path_ + ": truncated BAM record at the end of the file"); return false; }
      const uint32_t bsz = rd32(at());
      if (bsz < 32) throw Error(path_ + ": corrupt BAM record (block_size " + std::to_string(bsz) + ")");
      if (!need(4 + (size_t)std::min<uint32_t>(bsz, 32))) throw Error(path_ + ": truncated BAM record at the end of the file");
      const uint8_t* h = at() + 4;
      const size_t l_name = h[8], n_cigar = rd16(h + 12);
      const uint16_t flag = rd16(h + 14);
      const int32_t l_seq = (int32_t)rd32(h + 16);
      if (l_seq < 0) throw Error(path_ + ": corrupt BAM record (negative l_seq)");
      if ((int64_t)l_seq > max_len_)
        throw Error(path_ + ": a read of " + std::to_string(l_seq) + " bases is longer than the limit of " + std::to_string(max_len_) + " bases");
      const size_t seq_bytes = ((size_t)l_seq + 1) / 2;
      if (l_name < 1 || 32 + l_name + 4 * n_cigar + seq_bytes + (size_t)l_seq > bsz) throw Error(path_ + ": corrupt BAM record (fields overrun block_size)");
      if (!need(4 + (size_t)bsz)) throw Error(path_ + ": truncated BAM record at the end of the file");
      h = at() + 4;
      pos_ += 4 + (size_t)bsz;
      if (skip_filtered_ && (flag & 0x900)) continue;
      r.name.assign((const char*)h + 32, l_name - 1);
      const size_t nul = r.name.find('\0');
      if (nul != std::string::npos) r.name.resize(nul);
      r.seq = h + 32 + l_name + 4 * n_cigar;
      r.l_seq = l_seq;
      r.qual = l_seq > 0 && r.seq[seq_bytes] != 0xFF ? r.seq + seq_bytes : nullptr;
      r.flag = flag;
      r.mm = r.ml = r.mn = AuxField{};
      if (want_tags_) {
        const auto keep = [&](const AuxField& f) {
          if (f.tag[0] != 'M') return;
          if (f.tag[1] == 'M') r.mm = f; else if (f.tag[1] == 'L') r.ml = f; else if (f.tag[1] == 'N') r.mn = f;
        };
        if (!aux_walk(r.seq + seq_bytes + (size_t)l_seq, h + bsz, keep)) throw Error(path_ + ": corrupt BAM record (aux fields) of read " + r.name);
      }
      return true;
    }
  }
  size_t blocks() const { return z_.blocks(); }
  bool eof_marker() const { return z_.eof_marker(); }

 private:
  const uint8_t* at() const { return buf_.data() + pos_; }
  // at least n inflated bytes from pos_ on in buf_, inflating further segments as needed; false if the file ends first
  bool need(size_t n) {
    while (end_ - pos_ < n) {
      if (z_.at_end()) return false;
      if (pos_) { memmove(buf_.data(), buf_.data() + pos_, end_ - pos_); end_ -= pos_; pos_ = 0; }
      end_ += z_.inflate_segment(buf_, end_);
    }
    return true;
  }
  void read_header() {
    if (z_.size() == 0 || !bgzf_block_size(z_.data(), z_.size())) throw Error(path_ + ": bad magic: not a BGZF file");
    if (!need(8) || memcmp(at(), "BAM\1", 4) != 0) throw Error(path_ + ": bad magic: not a BAM file");
    const int32_t l_text = (int32_t)rd32(at() + 4);
    if (l_text < 0) throw Error(path_ + ": corrupt BAM header");
    if (!need(8 + (size_t)l_text + 4)) throw Error(path_ + ": truncated BAM header");
    pos_ += 8 + (size_t)l_text;
    const int32_t n_ref = (int32_t)rd32(at());
    if (n_ref < 0) throw Error(path_ + ": corrupt BAM header");
    pos_ += 4;
    for (int32_t i = 0; i < n_ref; ++i) {
      if (!need(4)) throw Error(path_ + ": truncated BAM header");
      const int32_t l_name = (int32_t)rd32(at());
      if (l_name < 0) throw Error(path_ + ": corrupt BAM header");
      if (!need(8 + (size_t)l_name)) throw Error(path_ + ": truncated BAM header");
      pos_ += 8 + (size_t)l_name;
    }
  }

  std::string path_;
  int64_t max_len_;
  bool skip_filtered_, want_tags_;
  BgzfStream z_;
  std::vector<uint8_t> buf_; size_t pos_ = 0, end_ = 0;          // inflated bytes [pos_, end_) of buf_ not parsed yet
};

}  // namespace bam
