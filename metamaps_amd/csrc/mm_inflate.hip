// BGZF blocks inflated on the device (mm_bgzf_inflate): one wavefront (a 64-thread workgroup) per block, grid-striding over the blocks of a
// batch.  The decode core is mm_inflate.hpp, shared with the host build the CPU tests check against zlib.  DESIGN.md §1 has the shape and
// what it costs.
//
// LDS per workgroup: the block's output (up to 64 KiB, placed at the global destination's offset mod 16 so the write-back is 16-byte
// stores), the two Huffman tables and the code lengths (~6 KiB) and a copy of the constant tables (~1.4 KiB: the CRC table lookups are a
// dependent chain, LDS latency instead of a global load per byte) and a 4 KiB ring of the block's compressed bytes.  ~77 KiB: two workgroups
// per CU.
#include "mm_codec.hpp"
#include "mm_inflate.hpp"
#include "mm_wave_lanes.hpp"
#include <algorithm>

namespace {

__constant__ mmi::Consts k_consts = mmi::make_consts();

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_off,
                                                          const int32_t* __restrict__ comp_len, int32_t n, uint8_t* __restrict__ out,
                                                          int64_t out_cap, const int64_t* __restrict__ out_off, int32_t* __restrict__ status) {
  __shared__ mmi::Consts K;
  __shared__ mmi::Scratch S;
  __shared__ __attribute__((aligned(16))) uint8_t buf[mmi::MAX_ISIZE + 16];
  __shared__ uint8_t ring[mmi::RING];
  {
    static_assert(sizeof(mmi::Consts) % 4 == 0, "");
    const uint32_t* src = (const uint32_t*)&k_consts;
    uint32_t* dst = (uint32_t*)&K;
    for (uint32_t i = threadIdx.x; i < sizeof(mmi::Consts) / 4; i += 64) dst[i] = src[i];
    __syncthreads();
  }
  mmi::WaveLanes p;
  p.ring = ring;
  for (int32_t b = blockIdx.x; b < n; b += gridDim.x) {
    const int64_t oo = out_off[b];
    uint8_t* const stage = buf + (oo & 15);                      // (same alignment mod 16 as the destination)
    uint32_t isize = 0;
    int32_t st = mmi::inflate_bgzf(p, S, K, comp + comp_off[b], (uint32_t)comp_len[b], stage, &isize);
    if (st == mmi::OK && (oo < 0 || oo + (int64_t)isize > out_cap)) st = mmi::BAD_LENGTH;   // (the host checked this; never write outside)
    if (st == mmi::OK) {
      uint8_t* const dst = out + oo;
      const uint32_t head = std::min<uint32_t>(isize, (uint32_t)((16 - (oo & 15)) & 15));
      for (uint32_t i = threadIdx.x; i < head; i += 64) dst[i] = stage[i];
      const uint32_t nvec = (isize - head) >> 4;
      const uint4* vs = (const uint4*)(stage + head);
      uint4* vd = (uint4*)(dst + head);
      for (uint32_t i = threadIdx.x; i < nvec; i += 64) vd[i] = vs[i];
      for (uint32_t i = head + (nvec << 4) + threadIdx.x; i < isize; i += 64) dst[i] = stage[i];
    }
    if (threadIdx.x == 0) status[b] = st;
    __syncthreads();                                             // (the next block reuses the staging)
  }
}

}  // namespace

namespace mm {

// Blocks whose inflated bytes stay on the device: the host's block[i] (comp_len[i] bytes) goes to d_out + out_off[i]; the caller has checked that every block's
// ISIZE bytes lie inside d_out[0, out_cap) (the kernel checks it again and never writes outside).  status[i] as mm_bgzf_inflate's; returns the
// number of blocks that are not ok, when the bytes are there.
int64_t bgzf_inflate_resident(mm_ctx* ctx, const uint8_t* const* block, const int32_t* comp_len, int32_t n, uint8_t* d_out, int64_t out_cap, const int64_t* out_off,
                              int32_t* status) {
  if (n == 0) return 0;
  hipStream_t st = ctx->stream;
  std::vector<int64_t> rel((size_t)n);
  int64_t cbytes = 0;
  for (int32_t i = 0; i < n; ++i) { rel[(size_t)i] = cbytes; cbytes += comp_len[i]; }
  uint8_t* const up = (uint8_t*)ctx->pinned_up_at_least(std::max<size_t>((size_t)cbytes, 1));
  for (int32_t i = 0; i < n; ++i) memcpy(up + rel[(size_t)i], block[i], (size_t)comp_len[i]);
  DBuf<uint8_t> d_comp(std::max<size_t>((size_t)cbytes, 1));
  d_comp.upload(up, (size_t)cbytes, st);
  DBuf<int64_t> d_off((size_t)n), d_oo((size_t)n);
  DBuf<int32_t> d_len((size_t)n), d_st((size_t)n);
  d_off.upload(rel.data(), (size_t)n, st); d_len.upload(comp_len, (size_t)n, st); d_oo.upload(out_off, (size_t)n, st);
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)std::max(1, ctx->cus) * 2);
  bgzf_inflate_kernel<<<dim3(grid), dim3(64), 0, st>>>(d_comp.p, d_off.p, d_len.p, n, d_out, out_cap, d_oo.p, d_st.p);
  MM_KERNEL_CHECK();
  d_st.download(status, (size_t)n, st);
  MM_HIP(mm::stream_sync(st));
  int64_t bad = 0;
  for (int32_t i = 0; i < n; ++i) bad += status[i] != mmi::OK;
  return bad;
}

// mm_bgzf_inflate's body: the number of blocks whose status is not ok.  Argument errors throw MM_ERR_ARG.
int64_t bgzf_inflate(mm_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, const int64_t* comp_off, const int32_t* comp_len, int32_t n,
                     uint8_t* out, int64_t out_cap, const int64_t* out_off, int32_t* status) {
  if (n == 0) return 0;
  hipStream_t st = ctx->stream;
  std::vector<uint32_t> isize((size_t)n, 0);                     // what each block says it inflates to (0 where it cannot be read)
  int64_t lo = comp_bytes, hi = 0, out_end = 0;
  for (int32_t i = 0; i < n; ++i) {
    MM_REQUIRE(comp_off[i] >= 0 && comp_len[i] >= 0 && comp_off[i] + comp_len[i] <= comp_bytes, MM_ERR_ARG,
               "mm_bgzf_inflate: block " + std::to_string(i) + " lies outside the compressed buffer");
    lo = std::min(lo, comp_off[i]); hi = std::max(hi, comp_off[i] + comp_len[i]);
    if (comp_len[i] >= 26) {
      const uint32_t s = mmi::rd32(comp + comp_off[i] + comp_len[i] - 4);
      if (s <= mmi::MAX_ISIZE) {
        isize[(size_t)i] = s;
        MM_REQUIRE(out_off[i] >= 0 && out_off[i] + (int64_t)s <= out_cap, MM_ERR_ARG,
                   "mm_bgzf_inflate: block " + std::to_string(i) + "'s ISIZE bytes do not fit the output at its offset");
        out_end = std::max(out_end, out_off[i] + (int64_t)s);
      }
    }
  }
  if (hi < lo) lo = hi = 0;
  const size_t cbytes = (size_t)(hi - lo);
  const size_t nthr = (size_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)std::max(1u, mm::cpu_budget() / 2), 16, (uint64_t)(std::max<size_t>(cbytes, (size_t)out_end) >> 23) + 1}));
  auto par = [&](const std::function<void(size_t, size_t)>& fn) {   // fn(t, nthr) on up to 16 threads: the host copies of large batches
    if (nthr > 1) { if (!ctx->pack_pool) ctx->pack_pool = std::make_unique<TaskPool>(31); ctx->pack_pool->run(nthr, [&](size_t t) { fn(t, nthr); }); }
    else fn(0, 1);
  };
  uint8_t* const up = (uint8_t*)ctx->pinned_up_at_least(std::max<size_t>(cbytes, 1));
  par([&](size_t t, size_t T) { const size_t a = cbytes * t / T, b = cbytes * (t + 1) / T; if (b > a) memcpy(up + a, comp + lo + a, b - a); });
  DBuf<uint8_t> d_comp(std::max<size_t>(cbytes, 1));
  d_comp.upload(up, cbytes, st);
  std::vector<int64_t> rel(comp_off, comp_off + n);
  for (auto& r : rel) r -= lo;
  DBuf<int64_t> d_off((size_t)n), d_oo((size_t)n);
  DBuf<int32_t> d_len((size_t)n), d_st((size_t)n);
  d_off.upload(rel.data(), (size_t)n, st);
  d_len.upload(comp_len, (size_t)n, st);
  d_oo.upload(out_off, (size_t)n, st);
  DBuf<uint8_t> d_out(std::max<size_t>((size_t)out_end, 1));
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)std::max(1, ctx->cus) * 2);
  bgzf_inflate_kernel<<<dim3(grid), dim3(64), 0, st>>>(d_comp.p, d_off.p, d_len.p, n, d_out.p, out_end, d_oo.p, d_st.p);
  MM_KERNEL_CHECK();
  std::vector<int32_t> sts((size_t)n);
  d_st.download(sts.data(), (size_t)n, st);
  uint8_t* const down = (uint8_t*)ctx->pinned_at_least(std::max<size_t>((size_t)out_end, 1));
  d_out.download(down, (size_t)out_end, st);
  MM_HIP(mm::stream_sync(st));
  // the ok blocks' bytes to the caller, runs of adjacent blocks in one piece; nothing else of `out` is written
  std::vector<std::pair<int64_t, int64_t>> runs;
  int64_t bad = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (status) status[i] = sts[(size_t)i];
    if (sts[(size_t)i] != mmi::OK) { ++bad; continue; }
    const int64_t a = out_off[i], b = a + isize[(size_t)i];
    if (b == a) continue;
    if (!runs.empty() && runs.back().second == a) runs.back().second = b;
    else runs.emplace_back(a, b);
  }
  for (auto& r : runs) {
    const size_t len = (size_t)(r.second - r.first);
    if (len < ((size_t)8 << 20)) { memcpy(out + r.first, down + r.first, len); continue; }
    par([&](size_t t, size_t T) { const size_t a = len * t / T, b = len * (t + 1) / T; if (b > a) memcpy(out + r.first + a, down + r.first + a, b - a); });
  }
  return bad;
}

}  // namespace mm
