// BAM records of aligned mappings, encoded and deflated on the device (mm_bam_encode; mapDirectly --bam; DESIGN.md section 1, "BAM output"; the record
// and its checks: mm_bam_core.hpp, the text the host test runs).
//   size     bam_size_kernel: one wavefront (a 64-thread workgroup) per job walks the job's runs once: the checks' sums and the MD text's length give
//            the record's exact size, 0 for a job without a record.  A job that breaks a rule puts (job << 4 | rule) into the error word with an
//            atomic minimum; the host reads the word before anything else is launched.
//   offsets  an exclusive scan of the sizes (mm_prims.hpp).  The host reads them back and cuts the jobs into groups whose records fit group_bytes.
//   write    bam_write_kernel: one wavefront per record of the group; the lanes share the name, the run words, the nibble-packed bases, the
//            qualities (the bytes of the reads' quality plane where the set has one, 0xFF otherwise) and the pieces of the MD
//            text.  Records start at any byte offset: everything is stored by bytes, 64 neighbouring ones per
//            store of the wavefront.
//   deflate  the group's records are the input of bgzf_deflate_kernel where they lie (mm_deflate.hip: bgzf_deflate_resident); only the members come
//            to the host.  One buffer of the largest group's size serves every group.
//   sorted   mm_bam_encode_sorted: between size and offsets, bam_key_kernel gives every job the key contig << 32 | first (a job without a record: the
//            key above every contig's), a stable radix sort of (key, job) gives slot -> job, bam_slot_size_kernel gathers the sizes in that order, and
//            the scan, the groups and the write kernel go by slot.  mm_bam_encode has no slot table: slot and job are the same number.
// No kernel here has an atomic other than the error word's, a barrier between workgroups or a loop that waits for another workgroup.
// The runs are the caller's (mm_alignment is a host object) and are uploaded whole: 4 bytes per run against the 27 KB of a 10 kb read's record.
// The jobs' arrays, their checks, the launch loop and the error word are mm_jobs_dev.hpp's, shared with mm_pileup.hip and mm_vcf.hip; flag, mapq and the
// names are this file's own columns (BamColumns).
#include "mm_bam.hpp"
#include "mm_bam_core.hpp"
#include "mm_deflate.hpp"
#include "mm_jobs_dev.hpp"
#include "mm_prims.hpp"

namespace mm {

__global__ void __launch_bounds__(64) bam_size_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len, int64_t n_contigs, AlignedJobs J,
                                                      BamColumns C, int64_t job0, int64_t* __restrict__ sizes, unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  WaveLanes p;
  const int32_t read = J.read[job], contig = J.contig[job], dist = J.dist[job];
  int rule = mmb::check_set(read, n_reads, contig, n_contigs);
  int64_t size = 0;
  if (!rule && dist >= 0 && q_len[read] > 0) {
    const int64_t l_name = C.name_off[job + 1] - C.name_off[job], n_ops = J.op_off[job + 1] - J.op_off[job], first = J.first[job];
    rule = mmb::check_head(J.strand[job], C.flag[job], l_name);
    if (!rule) {
      const mmb::Walk w = mmb::md_walk<false>(p, SeqBytes{}, J.ops + J.op_off[job], n_ops, first, nullptr);   // (sizing reads no reference byte)
      rule = mmb::check_walk(w, q_len[read], first, r_len[contig], dist);
      if (!rule) size = mmb::record_size(l_name, q_len[read], n_ops, w.md_len);
    }
  }
  if (threadIdx.x == 0) {
    sizes[job] = size;
    if (rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
  }
}

// (sorted alone) the order's key of every job, and the sizes in the order of the slots
__global__ void __launch_bounds__(256) bam_key_kernel(AlignedJobs J, const int64_t* __restrict__ sizes, uint64_t no_record, uint64_t* __restrict__ key) {
  const int64_t job = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (job >= J.n) return;
  key[job] = sizes[job] > 0 ? (uint64_t)J.contig[job] << 32 | (uint64_t)J.first[job] : no_record;   // (a record's first is in [0, 2^31): rule 6)
}
__global__ void __launch_bounds__(256) bam_slot_size_kernel(const int64_t* __restrict__ slot_job, const int64_t* __restrict__ sizes, int64_t n, int64_t* __restrict__ out) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot < n) out[slot] = sizes[slot_job[slot]];
}

// the records of the slots [slot0, slot1) of a group to raw + (off[slot] - off0); a slot of size 0 has none.  slot_job: the job of every slot, null
// where the slot is the job
__global__ void __launch_bounds__(64) bam_write_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, EditSeq R,
                                                       const uint64_t* __restrict__ r_base, const int32_t* __restrict__ r_len, AlignedJobs J, BamColumns C, int64_t slot0,
                                                       int64_t slot1, const int64_t* __restrict__ slot_job, const int64_t* __restrict__ off, int64_t off0,
                                                       const uint8_t* __restrict__ q_qual, uint8_t* __restrict__ raw) {
  const int64_t slot = slot0 + (int64_t)blockIdx.x;
  if (slot >= slot1 || off[slot + 1] == off[slot]) return;
  const int64_t job = slot_job ? slot_job[slot] : slot;
  WaveLanes p;
  const int32_t read = J.read[job], contig = J.contig[job];
  const uint64_t qg = q_base[read], rg = r_base[contig];
  mmb::Job j;
  j.ops = J.ops + J.op_off[job]; j.n_ops = J.op_off[job + 1] - J.op_off[job];
  j.name = C.names + C.name_off[job]; j.l_name = (int32_t)(C.name_off[job + 1] - C.name_off[job]);
  j.first = J.first[job]; j.m = q_len[read]; j.refid = contig; j.strand = J.strand[job]; j.dist = J.dist[job]; j.flag = C.flag[job]; j.mapq = C.mapq[job];
  mmb::write_record_q(p, j, SeqBytes{Q.narrowed(qg, qg + (uint64_t)j.m), (int64_t)qg, q_qual}, SeqBytes{R.narrowed(rg, rg + (uint64_t)r_len[contig]), (int64_t)rg}, raw + (off[slot] - off0));
}

void bam_encode_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& jobs_in, const BamColumns& in, int64_t group_bytes, bool sorted, BamMembers* out) {
  const char* const who = sorted ? "mm_bam_encode_sorted" : "mm_bam_encode";
  AlignedJobsDev jobs(ctx, reads, ref, jobs_in, who);
  MM_REQUIRE(group_bytes >= 0, MM_ERR_ARG, std::string(who) + ": a negative group_bytes");
  out->bgzf.clear(); out->rec_job.clear(); out->rec_off.assign(1, 0); out->n_records = 0; out->raw_bytes = 0;
  const int64_t n = jobs_in.n_jobs;
  if (n == 0) return;
  offsets_check(in.name_off, n, who, "name_off");
  const size_t k = (size_t)n, n_ops = jobs.n_ops, n_name = (size_t)in.name_off[n];
  MM_REQUIRE(n_name == 0 || in.names, MM_ERR_ARG, std::string(who) + ": a null array");
  hipStream_t st = ctx->stream;
  StageClock<5> clk(getenv("MM_BAM_TIMING") != nullptr, st);       // upload, size, scan, write, deflate (with the members' way to the host)

  clk.start();
  const AlignedJobs J = jobs.upload(st);
  DBuf<int64_t> d_name_off(k + 1), d_sizes(k + 1), d_off(k + 1);
  DBuf<uint16_t> d_flag(k); DBuf<uint8_t> d_mapq(k); DBuf<char> d_names(std::max<size_t>(n_name, 1));
  d_name_off.upload(in.name_off, k + 1, st); d_flag.upload(in.flag, k, st); d_mapq.upload(in.mapq, k, st); d_names.upload(in.names, n_name, st);
  d_sizes.zero(st);
  clk.stop(0);
  const BamColumns C{d_flag.p, d_mapq.p, d_name_off.p, d_names.p};

  clk.start();
  for_job_grids(0, n, [&](int64_t a, dim3 grid) {
    bam_size_kernel<<<grid, dim3(64), 0, st>>>(reads->d_len.p, reads->count(), ref->d_len.p, ref->count(), J, C, a, d_sizes.p, jobs.err.p);
  });
  jobs.require_no_error(st, mmb::rule_text);
  clk.stop(1);

  clk.start();
  DBuf<uint8_t> tmp;
  DBuf<int64_t> d_slot_job;                                        // sorted alone: the job of every slot
  std::vector<int64_t> slot_job;
  if (sorted) {
    const uint64_t n_contigs = (uint64_t)ref->count();
    DBuf<uint64_t> d_key(k), d_key_sorted(k); DBuf<int64_t> d_job(k), d_slot_sizes(k + 1);
    d_slot_job.alloc(k);
    bam_key_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(J, d_sizes.p, n_contigs << 32, d_key.p);
    MM_KERNEL_CHECK();
    fill_iota(d_job.p, n, st);
    sort_pairs(tmp, d_key.p, d_key_sorted.p, d_job.p, d_slot_job.p, k, 0, 32 + bits_for(n_contigs), st);   // (stable: equal keys stay in job order)
    d_slot_sizes.zero(st);
    bam_slot_size_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(d_slot_job.p, d_sizes.p, n, d_slot_sizes.p);
    MM_KERNEL_CHECK();
    exclusive_scan(tmp, d_slot_sizes.p, d_off.p, k + 1, st);
    slot_job = d_slot_job.to_host(st);
  } else {
    exclusive_scan(tmp, d_sizes.p, d_off.p, k + 1, st);
  }
  const std::vector<int64_t> off = d_off.to_host(st);
  clk.stop(2);
  out->raw_bytes = off[k];
  for (size_t i = 0; i < k; ++i)
    if (off[i + 1] > off[i]) { out->rec_job.push_back(sorted ? slot_job[i] : (int64_t)i); out->rec_off.push_back(off[i + 1]); }
  out->n_records = (int64_t)out->rec_job.size();

  // groups of consecutive slots whose records stay within gb; a record above gb is a group of its own
  const int64_t gb = group_bytes ? group_bytes : BAM_GROUP_BYTES;
  std::vector<int64_t> cut(1, 0);
  int64_t largest = 0;
  for (int64_t j0 = 0; j0 < n;) {
    int64_t j1 = j0, bytes = 0;
    for (; j1 < n; ++j1) { const int64_t s = off[(size_t)j1 + 1] - off[(size_t)j1]; if (bytes > 0 && bytes + s > gb) break; bytes += s; }
    cut.push_back(j1); largest = std::max(largest, bytes); j0 = j1;
  }
  if (largest == 0) return;
  DBuf<uint8_t> d_raw((size_t)largest + 16);                       // (the deflate kernel reads whole 16-byte pieces)
  out->bgzf.reserve((size_t)(out->raw_bytes / 3));
  std::vector<int32_t> sizes;
  for (size_t g = 0; g + 1 < cut.size(); ++g) {
    const int64_t j0 = cut[g], j1 = cut[g + 1], bytes = off[(size_t)j1] - off[(size_t)j0];
    if (bytes == 0) continue;
    clk.start();
    for_job_grids(j0, j1, [&](int64_t a, dim3 grid) {
      bam_write_kernel<<<grid, dim3(64), 0, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, edit_seq(ref), ref->d_base.p, ref->d_len.p, J, C, a, j1, d_slot_job.p, d_off.p,
                                                  off[(size_t)j0], reads->qual_ptr(), d_raw.p);
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
    fprintf(stderr, "MM_BAM_TIMING upload %.3f size %.3f scan %.3f write %.3f deflate %.3f ms; %lld jobs, %lld records, %lld runs, %zu groups, raw %lld B, bgzf %zu B\n", clk.ms[0], clk.ms[1],
            clk.ms[2], clk.ms[3], clk.ms[4], (long long)n, (long long)out->n_records, (long long)n_ops, cut.size() - 1, (long long)out->raw_bytes, out->bgzf.size());
}

}  // namespace mm
