// Homopolymer compression on the device (mapDirectly --hpc; DESIGN.md section 1, "Homopolymer compression").
//
// hpc(S) of every sequence of an uploaded set, as a set in the same layout, in five steps over the packed 2-bit stream:
//   1  run-start flags: one lane per 64 stream positions (four packed words, one 16-byte load) computes w ^ (w << 2 | prev >> 30) per word
//      (mm_hpc_core.hpp); the previous word's last base comes from the lane below (the wave's first lane reads it).  The result IS the
//      coordinate map's bitmap, 1 bit per raw stream position.
//   2  positions the codes cannot decide are rewritten in the bitmap: under exception runs (one wave per run: first base kept unless the
//      run continues an adjacent run of the same byte, the rest dropped, the base behind the run kept), the first base of every sequence
//      (kept) and the pad positions behind its last (dropped).
//   3  popcount per bitmap word, device-wide exclusive scan (mm_scan.hpp), rank of every sequence start -> compressed lengths and starts.
//   4  the write pass, one lane per OUTPUT word: the rank of its first base is known, a binary search over the scanned popcounts (inside
//      its sequence's words) finds the bitmap word that holds it, and the kept fields of the packed words from there on are extracted and
//      shifted into the word until it is full.  Every output word has one writer: no atomics on the output stream and nothing to merge
//      between tiles.
//   5  exception runs: a run whose first base is kept becomes a run of length 1 at the rank of its start (flag, scan, write).
// All indexes are 64-bit and all launches grid-stride.
#include "mm_hpc.hpp"
#include "mm_scan.hpp"
#include "mm_map.hpp"

namespace mm {
namespace {
constexpr int HPC_THREADS = 256;
inline unsigned hpc_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(std::max<int64_t>(items, 1), HPC_THREADS), 1 << 20)); }

// step 1
__global__ void __launch_bounds__(HPC_THREADS) hpc_flags_kernel(const uint32_t* __restrict__ packed, int64_t nwords, int64_t nb, int vec_ok, uint64_t* __restrict__ bitmap) {
  const int lane = threadIdx.x & 63;
  for (int64_t blk = blockIdx.x; blk * HPC_THREADS < nb; blk += gridDim.x) {   // (the whole block takes every turn: the shuffle below needs its lanes)
    const int64_t b = blk * HPC_THREADS + threadIdx.x, t = b << 2;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (b < nb) {
      if (vec_ok && t + 4 <= nwords) { const uint4 v = *(const uint4*)(packed + t); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
      else { for (int j = 0; j < 4; ++j) if (t + j < nwords) w[j] = packed[t + j]; }
    }
    uint32_t prev = __shfl_up(w[3], 1, 64);
    if (lane == 0) prev = (b > 0 && b < nb) ? packed[t - 1] : 0u;
    if (b < nb) {
      uint64_t m = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) m |= (uint64_t)hpc_keep_mask(w[j], (j ? w[j - 1] : prev) >> 30) << (16 * j);
      const int64_t valid = (nwords << 4) - (b << 6);              // stream positions of this word that exist
      if (valid < 64) m &= (1ull << valid) - 1;
      bitmap[b] = m;
    }
  }
}

__device__ __forceinline__ void hpc_clear_bits(uint32_t* bm32, uint64_t a, uint64_t e, int lane, int step) {   // bits [a, e), the words dealt out to `step` lanes
  if (e <= a) return;
  const uint64_t w0 = a >> 5, w1 = (e - 1) >> 5;
  for (uint64_t wi = w0 + (uint64_t)lane; wi <= w1; wi += (uint64_t)step) {
    uint32_t mask = ~0u;
    if (wi == w0) mask &= ~0u << (a & 31);
    if (wi == w1) mask &= ~0u >> (31 - ((e - 1) & 31));
    atomicAnd(&bm32[wi], ~mask);
  }
}

// step 2a: one wave per exception run
__global__ void __launch_bounds__(HPC_THREADS) hpc_exc_flags_kernel(const uint64_t* __restrict__ es, const uint32_t* __restrict__ el, const uint8_t* __restrict__ eb,
                                                                    int64_t n_exc, uint64_t total, uint32_t* __restrict__ bm32) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * HPC_THREADS + threadIdx.x) >> 6, nwaves = (int64_t)gridDim.x * (HPC_THREADS / 64);
  for (int64_t r = wave0; r < n_exc; r += nwaves) {
    const uint64_t s = es[r], e = s + el[r];
    if (e == s) continue;
    if (lane == 0) {
      const bool merged = r > 0 && es[r - 1] + el[r - 1] == s && eb[r - 1] == eb[r];   // (a sequence start is forced to "keep" by step 2b)
      if (merged) atomicAnd(&bm32[s >> 5], ~(1u << (s & 31))); else atomicOr(&bm32[s >> 5], 1u << (s & 31));
      const bool next_adjacent = r + 1 < n_exc && es[r + 1] == e;    // (that run decides its own first base)
      if (!next_adjacent && e < total) atomicOr(&bm32[e >> 5], 1u << (e & 31));   // (a pad position is cleared again by step 2b)
    }
    hpc_clear_bits(bm32, s + 1, e, lane, 64);
  }
}
// step 2b: one lane per sequence
__global__ void __launch_bounds__(HPC_THREADS) hpc_seq_flags_kernel(const uint64_t* __restrict__ base, const int32_t* __restrict__ len, int64_t n, uint32_t* __restrict__ bm32) {
  for (int64_t i = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * HPC_THREADS) {
    const uint64_t b0 = base[i], p0 = b0 + (uint64_t)len[i], p1 = base[i + 1];
    hpc_clear_bits(bm32, p0, p1, 0, 1);
    if (len[i] > 0) atomicOr(&bm32[b0 >> 5], 1u << (b0 & 31));
  }
}
// step 3
__global__ void __launch_bounds__(HPC_THREADS) hpc_count_kernel(const uint64_t* __restrict__ bitmap, int64_t nb, uint32_t* __restrict__ cnt) {
  for (int64_t b = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; b < nb; b += (int64_t)gridDim.x * HPC_THREADS) cnt[b] = (uint32_t)__popcll(bitmap[b]);
}
__global__ void __launch_bounds__(HPC_THREADS) hpc_seq_rank_kernel(const uint64_t* __restrict__ base, int64_t n, const uint64_t* __restrict__ bitmap,
                                                                   const uint64_t* __restrict__ bscan, uint64_t* __restrict__ seq_rank) {
  for (int64_t i = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * HPC_THREADS) seq_rank[i] = hpc_rank(bitmap, bscan, base[i]);
}

// the sequence that owns stream position g: base[i] <= g < base[i + 1] (g < base[n]; empty sequences own nothing)
__device__ __forceinline__ int64_t hpc_seq_of(const uint64_t* base, int64_t n, uint64_t g) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (base[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}
// the bitmap word that holds the set bit of rank r, among the words of the sequence that spans stream positions [g0, g1): bscan[b] <= r < bscan[b + 1]
__device__ __forceinline__ uint64_t hpc_word_of_rank(const uint64_t* bscan, uint64_t lo, uint64_t hi, uint64_t r) {
  while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (bscan[mid] <= r) lo = mid; else hi = mid; }
  return lo;
}

struct HpcStreams {
  const uint32_t* packed; const uint64_t* bitmap; const uint64_t* bscan;    // raw words, run-start bitmap, exclusive scan of its popcounts
  const uint64_t* base; const uint64_t* seq_rank;                           // raw sequence starts and their ranks [n + 1]
  const uint64_t* cbase; const int32_t* clen;                               // compressed starts [n + 1] and lengths
  int64_t n;
};

// step 4: one lane per output word
__global__ void __launch_bounds__(HPC_THREADS) hpc_write_kernel(HpcStreams S, int64_t cwords, uint32_t* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; q < cwords; q += (int64_t)gridDim.x * HPC_THREADS) {
    const int64_t i = hpc_seq_of(S.cbase, S.n, (uint64_t)q << 4);
    const int64_t j0 = (int64_t)(((uint64_t)q << 4) - S.cbase[i]);
    const int need = (int)min((int64_t)16, (int64_t)S.clen[i] - j0);
    uint64_t r = S.seq_rank[i] + (uint64_t)j0;                       // rank of the next base wanted
    const uint64_t hi = ((S.base[i + 1] - 1) >> 6) + 1;              // (bscan[hi] >= rank of the next sequence's start > r)
    uint64_t b = hpc_word_of_rank(S.bscan, S.base[i] >> 6, hi, r);
    uint64_t pre = S.bscan[b], acc = 0;                              // pre: rank of the first set bit not passed yet
    int fill = 0;
    while (fill < need) {
      const uint64_t bits = S.bitmap[b];
      if (bits == 0) { b = hpc_word_of_rank(S.bscan, b, hi, r); pre = S.bscan[b]; continue; }   // a long run: jump to the word of the next kept base
      for (int sub = 0; sub < 4 && fill < need; ++sub) {
        const uint32_t m16 = (uint32_t)(bits >> (16 * sub)) & 0xffffu;
        const int c = __popc(m16);
        if (pre + (uint64_t)c <= r) { pre += (uint64_t)c; continue; }
        int cc;
        uint32_t f = hpc_extract(S.packed[(b << 2) + (uint64_t)sub], m16, &cc);
        const int skip = (int)(r - pre);
        f >>= 2 * skip; cc -= skip;
        acc |= (uint64_t)f << (2 * fill);
        fill += cc; pre += (uint64_t)c; r = pre;
      }
      ++b;
    }
    if (need < 16) acc &= (1ull << (2 * need)) - 1;
    out[q] = (uint32_t)acc;
  }
}

// step 5
__global__ void __launch_bounds__(HPC_THREADS) hpc_exc_keep_kernel(const uint64_t* __restrict__ es, int64_t n_exc, const uint64_t* __restrict__ bitmap, uint32_t* __restrict__ keep) {
  for (int64_t r = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; r < n_exc; r += (int64_t)gridDim.x * HPC_THREADS) keep[r] = (uint32_t)((bitmap[es[r] >> 6] >> (es[r] & 63)) & 1ull);
}
__global__ void __launch_bounds__(HPC_THREADS) hpc_exc_write_kernel(HpcStreams S, const uint64_t* __restrict__ es, const uint8_t* __restrict__ eb, int64_t n_exc,
                                                                    const uint32_t* __restrict__ keep, const uint64_t* __restrict__ at, uint64_t* __restrict__ nes,
                                                                    uint32_t* __restrict__ nel, uint8_t* __restrict__ neb) {
  for (int64_t r = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; r < n_exc; r += (int64_t)gridDim.x * HPC_THREADS) {
    if (!keep[r]) continue;
    const int64_t i = hpc_seq_of(S.base, S.n, es[r]);
    nes[at[r]] = S.cbase[i] + (hpc_rank(S.bitmap, S.bscan, es[r]) - S.seq_rank[i]);
    nel[at[r]] = 1u; neb[at[r]] = eb[r];
  }
}

// the map's sampled select: raw position of kept base 512 s of sequence i
__global__ void __launch_bounds__(HPC_THREADS) hpc_sample_kernel(HpcStreams S, const uint64_t* __restrict__ samp_off, int64_t n_samp, uint32_t* __restrict__ samp) {
  for (int64_t t = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; t < n_samp; t += (int64_t)gridDim.x * HPC_THREADS) {
    const int64_t i = hpc_seq_of(samp_off, S.n, (uint64_t)t);
    const uint64_t r = S.seq_rank[i] + (((uint64_t)t - samp_off[i]) << HPC_SAMPLE_SHIFT);
    const uint64_t b = hpc_word_of_rank(S.bscan, S.base[i] >> 6, ((S.base[i + 1] - 1) >> 6) + 1, r);
    samp[t] = (uint32_t)((b << 6) + (uint64_t)hpc_select64(S.bitmap[b], (int)(r - S.bscan[b])) - S.base[i]);
  }
}

__global__ void __launch_bounds__(HPC_THREADS) hpc_to_raw_kernel(HpcMapView M, const int32_t* __restrict__ seq, const int64_t* __restrict__ pos, int64_t n,
                                                                 int64_t* __restrict__ first, int64_t* __restrict__ last) {
  for (int64_t t = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * HPC_THREADS) {
    first[t] = hpc_raw_first(M, seq[t], pos[t]);
    last[t] = hpc_raw_last(M, seq[t], pos[t]);
  }
}
__global__ void __launch_bounds__(HPC_THREADS) hpc_records_to_raw_kernel(HpcMapView M, mm_map_record* __restrict__ rec, int64_t n_rec, const int32_t* __restrict__ read_len,
                                                                         int64_t* __restrict__ end) {
  for (int64_t t = (int64_t)blockIdx.x * HPC_THREADS + threadIdx.x; t < n_rec; t += (int64_t)gridDim.x * HPC_THREADS) {
    const int64_t c = rec[t].ref_contig, start = rec[t].ref_start;
    if (c < 0 || c >= M.n) { end[t] = start + (int64_t)read_len[rec[t].read] - 1; continue; }   // (not a contig of this map: left as it is)
    end[t] = hpc_raw_last(M, c, start + (int64_t)read_len[rec[t].read] - 1);
    rec[t].ref_start = (int32_t)hpc_raw_first(M, c, start);
  }
}
}  // namespace

void seqset_hpc(mm_ctx* ctx, const mm_seqset* raw, mm_seqset* out, mm_hpc_map* map) {
  MM_REQUIRE(raw->frozen, MM_ERR_STATE, "sequence set not uploaded");
  MM_REQUIRE(raw->ctx->device == ctx->device, MM_ERR_ARG, "mm_seqset_hpc: the set lives on another device than the context");
  hipStream_t st = ctx->stream;
  const int64_t n = raw->count();
  const uint64_t total = raw->base[(size_t)n];
  const int64_t nwords = (int64_t)(total >> 4), nb = (int64_t)((total + 63) >> 6);
  // steps 1 and 2: the run-start bitmap (one word more than needed: a look-up may read the word behind the last position)
  DBuf<uint64_t> bitmap((size_t)nb + 1);
  MM_HIP(hipMemsetAsync(bitmap.p + nb, 0, sizeof(uint64_t), st));
  hpc_flags_kernel<<<dim3(hpc_grid(nb)), dim3(HPC_THREADS), 0, st>>>(raw->packed.p, nwords, nb, ((uintptr_t)raw->packed.p & 15) == 0 ? 1 : 0, bitmap.p);
  MM_KERNEL_CHECK();
  if (raw->n_exc) {
    hpc_exc_flags_kernel<<<dim3(hpc_grid(raw->n_exc * 64)), dim3(HPC_THREADS), 0, st>>>(raw->exc_start.p, raw->exc_len.p, raw->exc_byte.p, raw->n_exc, total, (uint32_t*)bitmap.p);
    MM_KERNEL_CHECK();
  }
  hpc_seq_flags_kernel<<<dim3(hpc_grid(n)), dim3(HPC_THREADS), 0, st>>>(raw->d_base.p, raw->d_len.p, n, (uint32_t*)bitmap.p);
  MM_KERNEL_CHECK();
  // step 3
  DBuf<uint32_t> cnt((size_t)std::max<int64_t>(nb, 1));
  DBuf<uint64_t> bscan((size_t)nb + 1), tmp, seq_rank((size_t)n + 1);
  hpc_count_kernel<<<dim3(hpc_grid(nb)), dim3(HPC_THREADS), 0, st>>>(bitmap.p, nb, cnt.p);
  MM_KERNEL_CHECK();
  exclusive_scan_u32_u64(cnt.p, nb, bscan.p, tmp, st);
  hpc_seq_rank_kernel<<<dim3(hpc_grid(n + 1)), dim3(HPC_THREADS), 0, st>>>(raw->d_base.p, n, bitmap.p, bscan.p, seq_rank.p);
  MM_KERNEL_CHECK();
  const std::vector<uint64_t> h_rank = seq_rank.to_host(st);
  out->len.resize((size_t)n); out->base.assign((size_t)n + 1, 0); out->total_bases = 0;
  std::vector<uint64_t> samp_off((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t cl = h_rank[(size_t)i + 1] - h_rank[(size_t)i];
    out->len[(size_t)i] = (int32_t)cl;
    out->base[(size_t)i + 1] = out->base[(size_t)i] + ((cl + 15) & ~15ull);
    out->total_bases += (int64_t)cl;
    samp_off[(size_t)i + 1] = samp_off[(size_t)i] + ((cl + (1u << HPC_SAMPLE_SHIFT) - 1) >> HPC_SAMPLE_SHIFT);
  }
  const int64_t cwords = (int64_t)(out->base[(size_t)n] >> 4);
  out->d_base.alloc((size_t)n + 1); out->d_base.upload(out->base.data(), (size_t)n + 1, st);
  out->d_len.alloc(std::max<size_t>((size_t)n, 1)); out->d_len.upload(out->len.data(), (size_t)n, st);
  out->packed.alloc((size_t)cwords + 1);
  MM_HIP(hipMemsetAsync(out->packed.p + cwords, 0, sizeof(uint32_t), st));   // the pad word every set ends on
  const HpcStreams S{raw->packed.p, bitmap.p, bscan.p, raw->d_base.p, seq_rank.p, out->d_base.p, out->d_len.p, n};
  // step 4
  if (cwords) { hpc_write_kernel<<<dim3(hpc_grid(cwords)), dim3(HPC_THREADS), 0, st>>>(S, cwords, out->packed.p); MM_KERNEL_CHECK(); }
  // step 5
  out->n_exc = 0;
  if (raw->n_exc) {
    DBuf<uint32_t> keep((size_t)raw->n_exc);
    DBuf<uint64_t> at((size_t)raw->n_exc + 1);
    hpc_exc_keep_kernel<<<dim3(hpc_grid(raw->n_exc)), dim3(HPC_THREADS), 0, st>>>(raw->exc_start.p, raw->n_exc, bitmap.p, keep.p);
    MM_KERNEL_CHECK();
    exclusive_scan_u32_u64(keep.p, raw->n_exc, at.p, tmp, st);
    uint64_t kept = 0;
    MM_HIP(hipMemcpyAsync(&kept, at.p + raw->n_exc, sizeof kept, hipMemcpyDeviceToHost, st));
    MM_HIP(mm::stream_sync(st));
    if (kept) {
      out->exc_start.alloc((size_t)kept); out->exc_len.alloc((size_t)kept); out->exc_byte.alloc((size_t)kept);
      hpc_exc_write_kernel<<<dim3(hpc_grid(raw->n_exc)), dim3(HPC_THREADS), 0, st>>>(S, raw->exc_start.p, raw->exc_byte.p, raw->n_exc, keep.p, at.p, out->exc_start.p,
                                                                                      out->exc_len.p, out->exc_byte.p);
      MM_KERNEL_CHECK();
      out->n_exc = (int64_t)kept;
    }
    MM_HIP(mm::stream_sync(st));                                   // (the temporaries of this block are released behind the kernels)
  }
  if (map) {
    map->ctx = ctx; map->n = n; map->rawlen = raw->len; map->clen = out->len;
    const int64_t n_samp = (int64_t)samp_off[(size_t)n];
    map->d_samp_off.alloc((size_t)n + 1); map->d_samp_off.upload(samp_off.data(), (size_t)n + 1, st);
    map->samp.alloc((size_t)std::max<int64_t>(n_samp, 1));
    if (n_samp) { hpc_sample_kernel<<<dim3(hpc_grid(n_samp)), dim3(HPC_THREADS), 0, st>>>(S, map->d_samp_off.p, n_samp, map->samp.p); MM_KERNEL_CHECK(); }
    map->d_base.alloc((size_t)n + 1); map->d_base.upload(raw->base.data(), (size_t)n + 1, st);
    map->d_rawlen.alloc(std::max<size_t>((size_t)n, 1)); map->d_rawlen.upload(raw->len.data(), (size_t)n, st);
    map->d_clen.alloc(std::max<size_t>((size_t)n, 1)); map->d_clen.upload(out->len.data(), (size_t)n, st);
    MM_HIP(mm::stream_sync(st));
    map->bitmap = std::move(bitmap);
  }
  MM_HIP(mm::stream_sync(st));
  out->frozen = true; out->hpc = true;
}

void hpc_map_to_raw(mm_hpc_map* map, const int32_t* seq, const int64_t* pos, int64_t n, int64_t* first_out, int64_t* last_out) {
  if (n <= 0) return;
  for (int64_t t = 0; t < n; ++t) MM_REQUIRE(seq[t] >= 0 && seq[t] < map->n, MM_ERR_ARG, "mm_hpc_map_to_raw: sequence index out of range");
  hipStream_t st = map->ctx->stream;
  DBuf<int32_t> d_seq((size_t)n); DBuf<int64_t> d_pos((size_t)n), d_first((size_t)n), d_last((size_t)n);
  d_seq.upload(seq, (size_t)n, st); d_pos.upload(pos, (size_t)n, st);
  hpc_to_raw_kernel<<<dim3(hpc_grid(n)), dim3(HPC_THREADS), 0, st>>>(map->view(), d_seq.p, d_pos.p, n, d_first.p, d_last.p);
  MM_KERNEL_CHECK();
  d_first.download(first_out, (size_t)n, st); d_last.download(last_out, (size_t)n, st);
  MM_HIP(mm::stream_sync(st));
}

void mapping_to_raw(mm_ctx* ctx, mm_mapping* m, const mm_hpc_map* ref_map, int64_t* end_out, int64_t cap) {
  MM_REQUIRE(ref_map->ctx->device == ctx->device && m->ctx->device == ctx->device, MM_ERR_ARG, "mm_mapping_to_raw: mapping, map and context live on different devices");
  MM_REQUIRE(cap >= m->n_rec, MM_ERR_ARG, "output capacity too small");
  MM_REQUIRE((int64_t)m->read_len.size() == m->n_reads, MM_ERR_STATE, "mm_mapping_to_raw: the mapping carries no read lengths");
  if (m->n_rec == 0) return;
  hipStream_t st = ctx->stream;
  DBuf<int32_t> d_len((size_t)std::max<int64_t>(m->n_reads, 1));
  d_len.upload(m->read_len.data(), (size_t)m->n_reads, st);
  DBuf<int64_t> d_end((size_t)m->n_rec);
  hpc_records_to_raw_kernel<<<dim3(hpc_grid(m->n_rec)), dim3(HPC_THREADS), 0, st>>>(ref_map->view(), m->rec.p, m->n_rec, d_len.p, d_end.p);
  MM_KERNEL_CHECK();
  d_end.download(end_out, (size_t)m->n_rec, st);
  MM_HIP(mm::stream_sync(st));
}

}  // namespace mm
