// FASTQ / FASTA records of selected reads of a resident set, written and deflated on the device (mm_reads_encode; mapDirectly --extract-* and
// --deplete-taxa; DESIGN.md section 1, "Read extraction"; the record and its rules: mm_reads_out_core.hpp, the text the host test runs).  The stages are
// mm_bam.hip's, without the alignment:
//   size     reads_size_kernel: one thread per record applies the three rules and gives the record's exact size.  A record that breaks a rule puts
//            (record << 4 | rule) into the error word with an atomic minimum; the host reads the word before anything else is launched.
//   offsets  an exclusive scan of the sizes (mm_prims.hpp).  The host reads them back and cuts the records into groups that fit group_bytes.
//   write    reads_write_kernel: one wavefront (a 64-thread workgroup) per record of the group.  A record starts at any byte offset, so each of the two
//            long stretches, bases and qualities, is written as up to three head bytes, aligned 4-byte words, 64 neighbouring ones per store of the
//            wavefront, and up to three tail bytes.  A word of bases is four 2-bit codes cut out of one or two packed words (EditSeq::bytes4), or four
//            bytes looked up one by one where an exception run of the read touches it; a read without exception runs (the common one: narrowed() leaves
//            it none) never searches.  A word of qualities is two aligned words of the plane shifted together, + 33 in every byte, '!' for 0xFF.  No
//            LDS: every lane's word depends on its own source words alone, and the stores of a wavefront are contiguous as they are.
//   deflate  the group's records are the input of bgzf_deflate_kernel where they lie (mm_deflate.hip: bgzf_deflate_resident); only the members come
//            to the host.  One buffer of the largest group's size serves every group.
// No kernel here has an atomic other than the error word's, a barrier between workgroups or a loop that waits for another workgroup.
#include "mm_reads_out.hpp"
#include "mm_reads_out_core.hpp"
#include "mm_bam.hpp"                                              // (BAM_GROUP_BYTES)
#include "mm_deflate.hpp"
#include "mm_jobs_dev.hpp"
#include "mm_prims.hpp"

namespace mm {

struct ReadsRecords { int64_t n; const int32_t* read; const int64_t* name_off; const char* names; };   // ReadsSelection on the device

__global__ void __launch_bounds__(256) reads_size_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, ReadsRecords S, int with_qual, int64_t* __restrict__ sizes,
                                                         unsigned long long* __restrict__ err) {
  const int64_t rec = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (rec >= S.n) return;
  const int64_t read = S.read[rec], l_name = S.name_off[rec + 1] - S.name_off[rec];
  const int rule = mmr::check(read, n_reads, S.names + S.name_off[rec], l_name);
  sizes[rec] = rule ? 0 : mmr::record_size(l_name, q_len[read], with_qual != 0);
  if (rule) atomicMin(err, (unsigned long long)rec << 4 | (unsigned long long)rule);
}

// m bytes at dst from word(i), the four bytes i .. i + 3 of the stretch as one little-endian word (asked only for i + 4 <= m), and byte(i): head bytes up
// to the first 4-byte boundary of dst, aligned words, tail bytes
template <class Word, class Byte> __device__ void put_stretch(uint8_t* dst, int64_t m, Word&& word, Byte&& byte) {
  const int64_t head = std::min<int64_t>(m, (int64_t)((0 - (uintptr_t)dst) & 3)), n_words = (m - head) >> 2, tail = head + 4 * n_words;
  if ((int64_t)threadIdx.x < head) dst[threadIdx.x] = byte((int64_t)threadIdx.x);
  for (int64_t k = threadIdx.x; k < n_words; k += 64) *reinterpret_cast<uint32_t*>(dst + head + 4 * k) = word(head + 4 * k);
  if (tail + (int64_t)threadIdx.x < m) dst[tail + threadIdx.x] = byte(tail + (int64_t)threadIdx.x);
}

// four stored qualities as their characters: + 33 in every byte, '!' for 0xFF (the only value with bit 7 set: a Phred value is 93 at most, so no byte carries)
__device__ uint32_t qual_chars4(uint32_t q) {
  const uint32_t none = ((q & 0x80808080u) >> 7) * 0xFFu;
  return (q & ~none) + 0x21212121u;
}

// the records [rec0, rec1) of a group to raw + (off[rec] - off0)
__global__ void __launch_bounds__(64) reads_write_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, const uint8_t* __restrict__ q_qual,
                                                         ReadsRecords S, int with_qual, int64_t rec0, int64_t rec1, const int64_t* __restrict__ off, int64_t off0,
                                                         uint8_t* __restrict__ raw) {
  const int64_t rec = rec0 + (int64_t)blockIdx.x;
  if (rec >= rec1) return;
  const int32_t read = S.read[rec];
  const int64_t g0 = (int64_t)q_base[read], m = q_len[read], l_name = S.name_off[rec + 1] - S.name_off[rec];
  const char* const name = S.names + S.name_off[rec];
  const SeqBytes src{Q.narrowed((uint64_t)g0, (uint64_t)(g0 + m)), g0, q_qual};
  const bool wq = with_qual != 0;
  uint8_t* const dst = raw + (off[rec] - off0);
  const int64_t b_at = mmr::bases_at(l_name), q_at = mmr::qual_at(l_name, m), size = mmr::record_size(l_name, m, wq);
  for (int64_t i = threadIdx.x; i < b_at; i += 64) dst[i] = mmr::record_byte(src, name, l_name, m, wq, i);             // '@' or '>', the name, '\n'
  put_stretch(dst + b_at, m, [&](int64_t i) { return src.s.bytes4(g0 + i); }, [&](int64_t i) { return src.byte(i); });
  const int64_t sep1 = wq ? q_at : size;                                                                               // '\n', and "+\n" before the qualities
  for (int64_t i = b_at + m + threadIdx.x; i < sep1; i += 64) dst[i] = mmr::record_byte(src, name, l_name, m, wq, i);
  if (!wq) return;
  if (q_qual) {
    const uint8_t* const plane = q_qual + g0;
    put_stretch(dst + q_at, m,
                [&](int64_t i) {
                  const uintptr_t a = (uintptr_t)(plane + i);
                  const uint32_t* const w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
                  const uint32_t sh = (uint32_t)(a & 3), lo = w[0], hi = sh ? w[1] : 0u;                             // (w[1] starts below plane[i + 3], inside the read's padded stretch)
                  return qual_chars4(__builtin_amdgcn_alignbyte(hi, lo, sh));
                },
                [&](int64_t i) { return mmr::qual_char(plane[i]); });
  } else {
    put_stretch(dst + q_at, m, [](int64_t) { return 0x21212121u; }, [](int64_t) { return (uint8_t)'!'; });
  }
  if (threadIdx.x == 0) dst[size - 1] = '\n';
}

void reads_encode_run(mm_ctx* ctx, const mm_seqset* reads, const ReadsSelection& sel, bool with_qual, int64_t group_bytes, ReadsText* out) {
  const char* const who = "mm_reads_encode";
  MM_REQUIRE(reads->frozen, MM_ERR_STATE, std::string(who) + ": the sequence set is not uploaded");
  MM_REQUIRE(!reads->hpc, MM_ERR_STATE, std::string(who) + ": the set is a result of mm_seqset_hpc: it does not hold the reads' own bases");
  MM_REQUIRE(reads->ctx->device == ctx->device, MM_ERR_ARG, std::string(who) + ": the sequence set lives on another device");
  MM_REQUIRE(group_bytes >= 0, MM_ERR_ARG, std::string(who) + ": a negative group_bytes");
  out->bgzf.clear(); out->n_records = 0; out->raw_bytes = 0;
  const int64_t n = sel.n;
  if (n == 0) return;
  offsets_check(sel.name_off, n, who, "name_off");
  const size_t k = (size_t)n, n_name = (size_t)sel.name_off[n];
  MM_REQUIRE(n_name == 0 || sel.names, MM_ERR_ARG, std::string(who) + ": a null array");
  hipStream_t st = ctx->stream;
  StageClock<5> clk(getenv("MM_READS_OUT_TIMING") != nullptr, st); // upload, size, scan, write, deflate (with the members' way to the host)

  clk.start();
  DBuf<int32_t> d_read(k); DBuf<int64_t> d_name_off(k + 1), d_sizes(k + 1), d_off(k + 1); DBuf<char> d_names(std::max<size_t>(n_name, 1));
  DBuf<unsigned long long> d_err(1);
  d_read.upload(sel.read, k, st); d_name_off.upload(sel.name_off, k + 1, st); d_names.upload(sel.names, n_name, st);
  d_sizes.zero(st);
  MM_HIP(hipMemsetAsync(d_err.p, 0xFF, sizeof(unsigned long long), st));
  clk.stop(0);
  const ReadsRecords S{n, d_read.p, d_name_off.p, d_names.p};

  clk.start();
  reads_size_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(reads->d_len.p, reads->count(), S, with_qual ? 1 : 0, d_sizes.p, d_err.p);
  MM_KERNEL_CHECK();
  const unsigned long long e = d_err.to_host(st)[0];              // read before anything else is launched: the write kernel trusts what this one checked
  MM_REQUIRE(e == JOB_NO_ERROR, MM_ERR_ARG, std::string(who) + ": record " + std::to_string(e >> 4) + ": " + mmr::rule_text((int)(e & 15)));
  clk.stop(1);

  clk.start();
  DBuf<uint8_t> tmp;
  exclusive_scan(tmp, d_sizes.p, d_off.p, k + 1, st);
  const std::vector<int64_t> off = d_off.to_host(st);
  clk.stop(2);
  out->raw_bytes = off[k]; out->n_records = n;

  // groups of consecutive records that stay within gb; a record above gb is a group of its own
  const int64_t gb = group_bytes ? group_bytes : BAM_GROUP_BYTES;
  std::vector<int64_t> cut(1, 0);
  int64_t largest = 0;
  for (int64_t j0 = 0; j0 < n;) {
    int64_t j1 = j0, bytes = 0;
    for (; j1 < n; ++j1) { const int64_t s = off[(size_t)j1 + 1] - off[(size_t)j1]; if (bytes > 0 && bytes + s > gb) break; bytes += s; }
    cut.push_back(j1); largest = std::max(largest, bytes); j0 = j1;
  }
  DBuf<uint8_t> d_raw((size_t)largest + 16);                       // (the deflate kernel reads whole 16-byte pieces)
  out->bgzf.reserve((size_t)(out->raw_bytes / 3));
  std::vector<int32_t> sizes;
  for (size_t g = 0; g + 1 < cut.size(); ++g) {
    const int64_t j0 = cut[g], j1 = cut[g + 1], bytes = off[(size_t)j1] - off[(size_t)j0];
    clk.start();
    for_job_grids(j0, j1, [&](int64_t a, dim3 grid) {
      reads_write_kernel<<<grid, dim3(64), 0, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, reads->qual_ptr(), S, with_qual ? 1 : 0, a, j1, d_off.p, off[(size_t)j0], d_raw.p);
    });
    clk.stop(3);
    clk.start();
    const int64_t nb = mmd::n_blocks_of(bytes);
    for (int64_t b0 = 0; b0 < nb; b0 += mmd::LAUNCH_BLOCKS) {
      const int64_t nblk = std::min(mmd::LAUNCH_BLOCKS, nb - b0), cbytes = std::min<int64_t>(nblk * mmd::BLOCK_IN, bytes - b0 * mmd::BLOCK_IN);
      uint8_t* const down = (uint8_t*)ctx->pinned_at_least((size_t)nblk * mmd::MEMBER_MAX);
      sizes.assign((size_t)nblk, 0);
      bgzf_deflate_resident(ctx, d_raw.p + b0 * mmd::BLOCK_IN, cbytes, nblk, down, sizes.data());
      for (int64_t b = 0; b < nblk; ++b) {
        MM_REQUIRE(sizes[(size_t)b] >= 26 && sizes[(size_t)b] <= (int32_t)mmd::BLOCK_IN + 31, MM_ERR_DEVICE, std::string(who) + ": a member's size is out of range");
        out->bgzf.insert(out->bgzf.end(), down + b * mmd::MEMBER_MAX, down + b * mmd::MEMBER_MAX + sizes[(size_t)b]);
      }
    }
    clk.stop(4);
  }
  if (clk.on)
    fprintf(stderr, "MM_READS_OUT_TIMING upload %.3f size %.3f scan %.3f write %.3f deflate %.3f ms; %lld records, %s, %zu groups, raw %lld B, bgzf %zu B\n", clk.ms[0], clk.ms[1], clk.ms[2],
            clk.ms[3], clk.ms[4], (long long)n, with_qual ? "FASTQ" : "FASTA", cut.size() - 1, (long long)out->raw_bytes, out->bgzf.size());
}

}  // namespace mm
