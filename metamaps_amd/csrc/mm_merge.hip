// Read-wise merge of the records of several index chunks, chunk order preserved (unifyFiles, mapWrap.h:128-132) — on the device.
// One part table, three sources of its bytes: mappings of this process (mapping_concat: resident, or a peer copy over xGMI), host arrays
// (mapping_from_parts), the ranks of a communicator (mapping_gather: ncclSend / ncclRecv).  DESIGN.md §4.
#include "mm_map.hpp"
#include <rccl/rccl.h>
#include "mm_prims.hpp"

namespace mm {
namespace {
struct PartDev { const uint64_t* off; const mm_map_record* rec; int32_t base; int32_t pad; };
__global__ void __launch_bounds__(256) merge_count_kernel(const PartDev* __restrict__ parts, int n_parts, int64_t n, uint64_t* __restrict__ cnt) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n) return;
  uint64_t c = 0;
  if (r < n) for (int p = 0; p < n_parts; ++p) c += parts[p].off[r + 1] - parts[p].off[r];
  cnt[r] = c;
}
__global__ void __launch_bounds__(256) merge_copy_kernel(const PartDev* __restrict__ parts, int n_parts, int64_t n, const uint64_t* __restrict__ off,
                                                         mm_map_record* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  uint64_t o = off[r];
  for (int p = 0; p < n_parts; ++p) {
    const PartDev P = parts[p];
    for (uint64_t i = P.off[r]; i < P.off[r + 1]; ++i) { mm_map_record x = P.rec[i]; x.ref_contig += P.base; out[o++] = x; }
  }
}

// The parts of one merge in chunk order, each n + 1 offsets and its records on the context's device, and the temporaries that hold what had to be brought there.
struct PartTable {
  mm_ctx* ctx; int64_t n;
  std::vector<PartDev> parts;
  std::vector<DBuf<uint64_t>> t_off; std::vector<DBuf<mm_map_record>> t_rec;
  PartTable(mm_ctx* c, int64_t n_reads, int n_parts) : ctx(c), n(n_reads) { parts.reserve((size_t)n_parts); t_off.reserve((size_t)n_parts); t_rec.reserve((size_t)n_parts); }
  void add_resident(const mm_mapping* P, int32_t base) { parts.push_back(PartDev{P->rec_off.p, P->rec.p, base, 0}); }
  void add_received(DBuf<uint64_t>&& off, DBuf<mm_map_record>&& rec, int32_t base) {
    t_off.push_back(std::move(off)); t_rec.push_back(std::move(rec));
    parts.push_back(PartDev{t_off.back().p, t_rec.back().p, base, 0});
  }
  void add_peer(const mm_mapping* P, int32_t base) {            // (the part's own stream has been waited for by the call that made it)
    DBuf<uint64_t> off((size_t)n + 1); DBuf<mm_map_record> rec(std::max<size_t>((size_t)P->n_rec, 1));
    MM_HIP(hipMemcpyPeerAsync(off.p, ctx->device, P->rec_off.p, P->ctx->device, sizeof(uint64_t) * ((size_t)n + 1), ctx->stream));
    if (P->n_rec > 0) MM_HIP(hipMemcpyPeerAsync(rec.p, ctx->device, P->rec.p, P->ctx->device, sizeof(mm_map_record) * (size_t)P->n_rec, ctx->stream));
    add_received(std::move(off), std::move(rec), base);
  }
  void add_host(const int64_t* off, const mm_map_record* rec, int32_t base) {
    const size_t nr = (size_t)off[n];
    DBuf<uint64_t> d_off((size_t)n + 1); d_off.upload((const uint64_t*)off, (size_t)n + 1, ctx->stream);
    DBuf<mm_map_record> d_rec(std::max<size_t>(nr, 1)); d_rec.upload(rec, nr, ctx->stream);
    add_received(std::move(d_off), std::move(d_rec), base);
  }
};

void merge_parts(mm_ctx* ctx, const std::vector<int32_t>& read_len, const mm_map_params& params, const PartTable& T, mm_mapping* M) {
  hipStream_t st = ctx->stream;
  const int64_t n = T.n;
  const std::vector<PartDev>& parts = T.parts;
  M->ctx = ctx; M->n_reads = n; M->params = params; M->read_len = read_len;
  M->active.assign((size_t)n, 0);
  M->stats = mm_map_stats{};
  M->stats.n_reads = n;
  for (int64_t r = 0; r < n; ++r) {
    const int L = read_len[(size_t)r];
    const bool ok = !(L < params.w || L < params.k || L < params.min_read_len);   // computeMap.hpp:137
    M->active[(size_t)r] = ok;
    if (ok) { M->stats.n_reads_long_enough++; M->stats.bases_long_enough += L; }
  }
  DBuf<PartDev> d_parts(parts.size()); d_parts.upload(parts.data(), parts.size(), st);
  DBuf<uint64_t> cnt((size_t)n + 1);
  M->rec_off.alloc((size_t)n + 1);
  const unsigned gb = (unsigned)ceil_div(n + 1, 256);
  merge_count_kernel<<<dim3(gb), dim3(256), 0, st>>>(d_parts.p, (int)parts.size(), n, cnt.p);
  MM_KERNEL_CHECK();
  DBuf<uint8_t> tmp;
  exclusive_scan(tmp, cnt.p, M->rec_off.p, (size_t)n + 1, st);
  M->h_rec_off = M->rec_off.to_host(st);
  M->n_rec = (int64_t)M->h_rec_off[(size_t)n];
  M->rec.alloc(std::max<size_t>((size_t)M->n_rec, 1));
  if (n > 0 && M->n_rec > 0) {
    merge_copy_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st>>>(d_parts.p, (int)parts.size(), n, M->rec_off.p, M->rec.p);
    MM_KERNEL_CHECK();
  }
  M->d_read_len.alloc((size_t)std::max<int64_t>(n, 1)); M->d_read_len.upload(M->read_len.data(), (size_t)n, st);
  M->stats.n_mappings = M->n_rec;
  for (int64_t r = 0; r < n; ++r) if (M->h_rec_off[(size_t)r + 1] > M->h_rec_off[(size_t)r]) M->stats.n_reads_mapped++;
  M->released = true;                                          // records only: the debug taps have nothing to show
  MM_HIP(stream_sync(st));
}
void add_part_stats(mm_mapping* M, mm_mapping* const* parts, int n_parts) {   // work counters and stage times: summed over the chunks; per-read facts: of chunk 0
  for (int p = 0; p < n_parts; ++p) {
    const mm_map_stats& S = parts[p]->stats;
    M->stats.sum_hits += S.sum_hits; M->stats.n_candidates += S.n_candidates; M->stats.sum_hits_kept += S.sum_hits_kept;
    M->stats.sum_l2_stream_entries += S.sum_l2_stream_entries; M->stats.sum_l2_evals += S.sum_l2_evals;
    M->stats.n_l2_rebuilds += S.n_l2_rebuilds; M->stats.n_l2_wide_redo += S.n_l2_wide_redo;
    M->stats.ms_minimizer += S.ms_minimizer; M->stats.ms_sketch += S.ms_sketch; M->stats.ms_probe_gather += S.ms_probe_gather;
    M->stats.ms_sort_hits += S.ms_sort_hits; M->stats.ms_l1_scan += S.ms_l1_scan; M->stats.ms_l2 += S.ms_l2; M->stats.ms_compact += S.ms_compact;
    M->stats.ms_total += S.ms_total; M->stats.ms_hit_filter += S.ms_hit_filter;
  }
  if (n_parts > 0) {
    M->stats.sum_sketch = parts[0]->stats.sum_sketch; M->stats.n_ambiguous_sketch_reads = parts[0]->stats.n_ambiguous_sketch_reads;
    M->stats.n_reads_giant = parts[0]->stats.n_reads_giant;
  }
}
void require_records(const mm_mapping* P, const char* who) {
  MM_REQUIRE(!P->sketch_only && P->rec_off.p && (P->n_rec == 0 || P->rec.p), MM_ERR_STATE, std::string(who) + ": a part holds no records (a mm_sketch_batch result is no chunk mapping)");
}
}  // namespace

// Parts may live in any context of this process: those of another DEVICE come over with a peer copy (xGMI), nothing is staged on the host.
void mapping_concat(mm_ctx* ctx, mm_mapping* const* parts, const int32_t* contig_base, int n_parts, mm_mapping* M) {
  PartTable T(ctx, parts[0]->n_reads, n_parts);
  for (int p = 0; p < n_parts; ++p) {
    const mm_mapping* P = parts[p];
    MM_REQUIRE(P->n_reads == T.n, MM_ERR_ARG, "chunk results cover different read sets");
    require_records(P, "mm_mapping_concat");
    const int32_t base = contig_base ? contig_base[p] : 0;
    if (P->ctx->device != ctx->device) T.add_peer(P, base); else T.add_resident(P, base);
  }
  merge_parts(ctx, parts[0]->read_len, parts[0]->params, T, M);
  add_part_stats(M, parts, n_parts);
}
void mapping_from_parts(mm_ctx* ctx, int64_t n_reads, const int32_t* read_len, const mm_map_params& params, int n_parts, const int64_t* const* offsets,
                        const mm_map_record* const* records, const int32_t* contig_base, mm_mapping* M) {
  PartTable T(ctx, n_reads, n_parts);
  for (int i = 0; i < n_parts; ++i) T.add_host(offsets[i], records[i], contig_base ? contig_base[i] : 0);
  merge_parts(ctx, std::vector<int32_t>(read_len, read_len + n_reads), params, T, M);
}

// The same exchange between the ranks of a communicator (one process per GPU, or one thread per GPU of one process): ncclSend / ncclRecv of the
// offsets, then of the records, straight between the devices.  Collective: every rank calls it for the same batch; true on the owner, which alone fills M.
bool mapping_gather(mm_ctx* ctx, int owner, int64_t n_reads, const int32_t* read_len, const mm_map_params& params, mm_mapping* const* parts, const int32_t* chunk_id,
                    int n_parts, int n_chunks, const int32_t* chunk_rank, const int32_t* contig_base, mm_mapping* M) {
  hipStream_t st = ctx->stream;
  const int rank = ctx->comm ? ctx->comm_rank : 0, nranks = ctx->comm ? ctx->comm_size : 1;
  MM_REQUIRE(owner >= 0 && owner < nranks, MM_ERR_ARG, "mm_mapping_gather: owner is no rank of the communicator");
  ncclComm_t comm = (ncclComm_t)ctx->comm;
  const bool self_send = getenv("MM_GATHER_SELF_SEND") != nullptr && comm;   // test hook: the owner's own parts go through ncclSend / ncclRecv too
  auto nccl_ok = [&](ncclResult_t rc, const char* what) { MM_REQUIRE(rc == ncclSuccess, MM_ERR_COMM, std::string(what) + ": " + ncclGetErrorString(rc)); };
  std::vector<int> part_of((size_t)n_chunks, -1);              // chunk -> index into parts[] (this rank's chunks)
  for (int i = 0; i < n_parts; ++i) {
    MM_REQUIRE(chunk_id[i] >= 0 && chunk_id[i] < n_chunks && chunk_rank[chunk_id[i]] == rank && parts[i] && parts[i]->n_reads == n_reads, MM_ERR_ARG, "mm_mapping_gather: a part is not a chunk of this rank");
    MM_REQUIRE(parts[i]->ctx->device == ctx->device, MM_ERR_ARG, "mm_mapping_gather: parts live on the rank's own device");
    require_records(parts[i], "mm_mapping_gather");
    part_of[(size_t)chunk_id[i]] = i;
  }
  for (int c = 0; c < n_chunks; ++c) MM_REQUIRE(chunk_rank[c] != rank || part_of[(size_t)c] >= 0, MM_ERR_ARG, "mm_mapping_gather: a chunk of this rank has no part");
  const size_t n1 = (size_t)n_reads + 1;
  if (rank != owner) {                                         // my chunks, ascending: all offset arrays, then all record arrays
    MM_REQUIRE(comm, MM_ERR_STATE, "mm_mapping_gather needs a communicator (mm_comm_init)");
    nccl_ok(ncclGroupStart(), "ncclGroupStart");
    for (int c = 0; c < n_chunks; ++c) if (chunk_rank[c] == rank) nccl_ok(ncclSend(parts[part_of[(size_t)c]]->rec_off.p, n1, ncclUint64, owner, comm, st), "ncclSend");
    nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
    nccl_ok(ncclGroupStart(), "ncclGroupStart");
    for (int c = 0; c < n_chunks; ++c) if (chunk_rank[c] == rank) { mm_mapping* P = parts[part_of[(size_t)c]]; if (P->n_rec > 0) nccl_ok(ncclSend(P->rec.p, sizeof(mm_map_record) * (size_t)P->n_rec, ncclInt8, owner, comm, st), "ncclSend"); }
    nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
    MM_HIP(stream_sync(st));
    return false;
  }
  std::vector<DBuf<uint64_t>> t_off((size_t)n_chunks); std::vector<DBuf<mm_map_record>> t_rec((size_t)n_chunks);
  auto remote = [&](int c) { return chunk_rank[c] != rank || self_send; };
  bool any_remote = false;
  for (int c = 0; c < n_chunks; ++c) any_remote = any_remote || remote(c);
  std::vector<uint64_t> n_rec_of((size_t)n_chunks, 0);
  if (any_remote) {
    MM_REQUIRE(comm, MM_ERR_STATE, "mm_mapping_gather needs a communicator (mm_comm_init)");
    nccl_ok(ncclGroupStart(), "ncclGroupStart");
    for (int c = 0; c < n_chunks; ++c) {
      if (!remote(c)) continue;
      t_off[(size_t)c].alloc(n1);
      if (chunk_rank[c] == rank) nccl_ok(ncclSend(parts[part_of[(size_t)c]]->rec_off.p, n1, ncclUint64, rank, comm, st), "ncclSend");
      nccl_ok(ncclRecv(t_off[(size_t)c].p, n1, ncclUint64, chunk_rank[c], comm, st), "ncclRecv");
    }
    nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
    for (int c = 0; c < n_chunks; ++c) if (remote(c)) t_off[(size_t)c].download(&n_rec_of[(size_t)c], 1, st, (size_t)n_reads);
    MM_HIP(stream_sync(st));
    nccl_ok(ncclGroupStart(), "ncclGroupStart");
    for (int c = 0; c < n_chunks; ++c) {
      if (!remote(c) || n_rec_of[(size_t)c] == 0) continue;
      t_rec[(size_t)c].alloc((size_t)n_rec_of[(size_t)c]);
      if (chunk_rank[c] == rank) nccl_ok(ncclSend(parts[part_of[(size_t)c]]->rec.p, sizeof(mm_map_record) * (size_t)n_rec_of[(size_t)c], ncclInt8, rank, comm, st), "ncclSend");
      nccl_ok(ncclRecv(t_rec[(size_t)c].p, sizeof(mm_map_record) * (size_t)n_rec_of[(size_t)c], ncclInt8, chunk_rank[c], comm, st), "ncclRecv");
    }
    nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
  }
  PartTable T(ctx, n_reads, n_chunks);
  for (int c = 0; c < n_chunks; ++c) {
    const int32_t base = contig_base ? contig_base[c] : 0;
    if (remote(c)) T.add_received(std::move(t_off[(size_t)c]), std::move(t_rec[(size_t)c]), base);
    else T.add_resident(parts[part_of[(size_t)c]], base);
  }
  merge_parts(ctx, std::vector<int32_t>(read_len, read_len + n_reads), params, T, M);
  add_part_stats(M, parts, n_parts);                           // (of the owner's own chunks: the counters of the other ranks stay with them)
  return true;
}

}  // namespace mm
