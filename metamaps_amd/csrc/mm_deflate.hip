// BGZF blocks deflated on the device (mm_bgzf_deflate): one wavefront (a 64-thread workgroup) per BGZF block of 65 280 input bytes,
// grid-striding over the blocks of a batch.  The encoder core is mm_deflate.hpp, shared with the host build the CPU tests check against
// zlib; what it writes does not depend on the grid or the device.  DESIGN.md §1 has the shape and what it costs.
//
// LDS per workgroup: the block's input (65 296 B: matches are measured in it, the CRC runs over it), 8 KiB that is the head table of 4 096
// 16-bit positions during the search, then the scratch of the code construction, then the 4 KiB window of output words; histograms, codes,
// the run-length coded code lengths and a step's matches (~4.6 KiB); a copy of the constant tables (~1.4 KiB: the CRC table lookups are a
// dependent chain).  ~79 KiB: two workgroups per CU.  The tokens of a block (4 B each, one per position at most) do not fit beside that:
// they go to a buffer in global memory, 255 KiB per resident workgroup, written once in rising order by the search and read once by the emit.
// Each member is written to a 64 KiB slot of its own (16-byte stores from the window); the host packs the members while it copies them
// out of the pinned staging.
#include "mm_codec.hpp"
#include "mm_deflate.hpp"
#include <zlib.h>
#include <algorithm>

namespace {

__constant__ mmi::Consts k_consts = mmi::make_consts();

struct DeflateLanes {
  static constexpr uint32_t W = 64;
  __device__ uint32_t lane() const { return threadIdx.x; }
  __device__ void sync() const { __syncthreads(); }
  __device__ uint32_t xor_all(uint32_t v) const {
#pragma unroll
    for (int o = 32; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
  }
  // every lane calls it (slot null: nothing to insert).  Lanes of one step may share a slot: they write until the slot holds the largest.
  __device__ void insert_max(uint16_t* slot, uint32_t v) const {
    for (;;) {
      const bool w = slot && *slot < v;
      if (__ballot(w) == 0) break;
      if (w) *slot = (uint16_t)v;
      __syncthreads();
    }
  }
  __device__ void add(uint32_t* a, uint32_t v) const { atomicAdd(a, v); }
  __device__ void or32(uint32_t* a, uint32_t v) const { atomicOr(a, v); }
  __device__ uint32_t scan_excl(uint32_t v, uint32_t* total) const {
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64); if ((int)threadIdx.x >= o) x += y; }
    *total = (uint32_t)__shfl((int)x, 63, 64);
    return x - v;
  }
};

// in: in_bytes bytes, 16-byte aligned, 16 readable bytes behind them.  Block b is in[b * BLOCK_IN, ...); its member goes to
// slots + b * MEMBER_MAX and its size to sizes[b].  tok: TOK_CAP words per workgroup of the grid.
__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t* __restrict__ in, int64_t in_bytes, int32_t n_blocks,
                                                          uint8_t* __restrict__ slots, uint32_t* __restrict__ tok, int32_t* __restrict__ sizes) {
  __shared__ mmi::Consts K;
  __shared__ mmd::Scratch S;
  {
    static_assert(sizeof(mmi::Consts) % 4 == 0, "");
    const uint32_t* src = (const uint32_t*)&k_consts;
    uint32_t* dst = (uint32_t*)&K;
    for (uint32_t i = threadIdx.x; i < sizeof(mmi::Consts) / 4; i += 64) dst[i] = src[i];
  }
  DeflateLanes p;
  uint32_t* const my_tok = tok + (size_t)blockIdx.x * mmd::TOK_CAP;
  for (int32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t at = (int64_t)b * mmd::BLOCK_IN;
    const uint32_t n = (uint32_t)std::min<int64_t>(mmd::BLOCK_IN, in_bytes - at);
    __syncthreads();                                             // (the last block's readers are done with S.in; K is written)
    const uint4* const vs = (const uint4*)(in + at);
    uint4* const vd = (uint4*)S.in;
    for (uint32_t i = threadIdx.x; i < (n + 15) / 16; i += 64) vd[i] = vs[i];
    __syncthreads();
    if (threadIdx.x < 16) S.in[n + threadIdx.x] = 0;
    __syncthreads();
    uint32_t stored;
    const uint32_t m = mmd::deflate_member(p, S, K, n, my_tok, slots + (size_t)b * mmd::MEMBER_MAX, &stored);
    if (threadIdx.x == 0) sizes[b] = (int32_t)m;
  }
}

// one block on the host with zlib level 1, in the same container (MM_DEFLATE_HOST); returns the member's bytes
uint32_t host_member(const uint8_t* in, uint32_t n, uint8_t* dst) {
  const uint8_t h[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0};
  memcpy(dst, h, 16);
  z_stream z;
  memset(&z, 0, sizeof z);
  uint32_t dn = 0;
  if (deflateInit2(&z, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK) {
    z.next_in = const_cast<Bytef*>(in); z.avail_in = n;
    z.next_out = dst + 18; z.avail_out = n + 4;                  // (anything that does not fit below the stored form is written stored)
    if (deflate(&z, Z_FINISH) == Z_STREAM_END) dn = (uint32_t)z.total_out;
    deflateEnd(&z);
  }
  if (!dn) {
    uint8_t* q = dst + 18;
    q[0] = 1; q[1] = (uint8_t)(n & 255); q[2] = (uint8_t)(n >> 8); q[3] = (uint8_t)(~n & 255); q[4] = (uint8_t)((~n >> 8) & 255);
    memcpy(q + 5, in, n);
    dn = n + 5;
  }
  const uint32_t member = 18 + dn + 8, crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, n);
  dst[16] = (uint8_t)((member - 1) & 255); dst[17] = (uint8_t)((member - 1) >> 8);
  uint8_t* t = dst + 18 + dn;
  for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)(n >> (8 * k)); }
  return member;
}

}  // namespace

namespace mm {

int64_t bgzf_deflate_bound(int64_t in_bytes) { return mmd::bound(in_bytes); }

// The blocks of input that already lies on the device: d_in holds in_bytes bytes (16-byte aligned, 16 readable bytes behind them), n blocks of
// BLOCK_IN bytes, mmd::LAUNCH_BLOCKS at most.  Member b comes back at down + b * MEMBER_MAX (host memory, pinned or not) with sizes[b] bytes;
// the input never visits the host.  Returns when both are there.
void bgzf_deflate_resident(mm_ctx* ctx, const uint8_t* d_in, int64_t in_bytes, int64_t n, uint8_t* down, int32_t* sizes) {
  hipStream_t st = ctx->stream;
  DBuf<uint8_t> d_slots((size_t)n * mmd::MEMBER_MAX);
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)std::max(1, ctx->cus) * 2);
  DBuf<uint32_t> d_tok((size_t)grid * mmd::TOK_CAP);
  DBuf<int32_t> d_sizes((size_t)n);
  bgzf_deflate_kernel<<<dim3(grid), dim3(64), 0, st>>>(d_in, in_bytes, (int32_t)n, d_slots.p, d_tok.p, d_sizes.p);
  MM_KERNEL_CHECK();
  d_sizes.download(sizes, (size_t)n, st);
  d_slots.download(down, (size_t)n * mmd::MEMBER_MAX, st);
  MM_HIP(mm::stream_sync(st));
}

// mm_bgzf_deflate's body.  Argument errors throw MM_ERR_ARG.
void bgzf_deflate(mm_ctx* ctx, const uint8_t* in, int64_t in_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int32_t* n_blocks) {
  MM_REQUIRE(in_bytes >= 0 && out_bytes && n_blocks && (in_bytes == 0 || (in && out)), MM_ERR_ARG, "mm_bgzf_deflate: null pointer or negative size");
  MM_REQUIRE(out_cap >= mmd::bound(in_bytes), MM_ERR_ARG,
             "mm_bgzf_deflate: out_cap " + std::to_string(out_cap) + " is below mm_bgzf_deflate_bound(" + std::to_string(in_bytes) + ") = " + std::to_string(mmd::bound(in_bytes)));
  MM_REQUIRE(mmd::n_blocks_of(in_bytes) <= INT32_MAX, MM_ERR_LIMIT, "mm_bgzf_deflate: more than 2^31 - 1 blocks");
  *out_bytes = 0; *n_blocks = 0;
  const int64_t nb = mmd::n_blocks_of(in_bytes);
  if (nb == 0) return;
  const size_t nthr = (size_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)std::max(1u, mm::cpu_budget() / 2), 16, (uint64_t)(in_bytes >> 20) + 1}));
  auto par = [&](size_t items, const std::function<void(size_t)>& fn) {   // fn(t) for t < items on up to 16 threads
    if (nthr > 1 && items > 1) { if (!ctx->pack_pool) ctx->pack_pool = std::make_unique<TaskPool>(31); ctx->pack_pool->run(items, fn); }
    else for (size_t t = 0; t < items; ++t) fn(t);
  };
  const char* const he = getenv("MM_DEFLATE_HOST");
  const bool host = he && *he && strcmp(he, "0") != 0;
  const int64_t CHUNK = mmd::LAUNCH_BLOCKS;
  std::vector<int32_t> sizes;
  std::vector<int64_t> offs;
  int64_t o = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += CHUNK) {
    const int64_t n = std::min(CHUNK, nb - b0);
    const uint8_t* const cin = in + b0 * mmd::BLOCK_IN;
    const int64_t cbytes = std::min<int64_t>(n * mmd::BLOCK_IN, in_bytes - b0 * mmd::BLOCK_IN);
    uint8_t* const down = (uint8_t*)ctx->pinned_at_least((size_t)n * mmd::MEMBER_MAX);
    sizes.assign((size_t)n, 0);
    if (host) {
      par(nthr, [&](size_t t) {
        for (size_t b = (size_t)n * t / nthr; b < (size_t)n * (t + 1) / nthr; ++b)
          sizes[b] = (int32_t)host_member(cin + b * mmd::BLOCK_IN, (uint32_t)std::min<int64_t>(mmd::BLOCK_IN, cbytes - (int64_t)b * mmd::BLOCK_IN), down + b * mmd::MEMBER_MAX);
      });
    } else {
      hipStream_t st = ctx->stream;
      uint8_t* const up = (uint8_t*)ctx->pinned_up_at_least((size_t)cbytes);
      par(nthr, [&](size_t t) { const size_t a = (size_t)cbytes * t / nthr, b = (size_t)cbytes * (t + 1) / nthr; if (b > a) memcpy(up + a, cin + a, b - a); });
      DBuf<uint8_t> d_in((size_t)cbytes + 16);
      d_in.upload(up, (size_t)cbytes, st);
      bgzf_deflate_resident(ctx, d_in.p, cbytes, n, down, sizes.data());
    }
    offs.resize((size_t)n);
    for (int64_t b = 0; b < n; ++b) {
      MM_REQUIRE(sizes[(size_t)b] >= 26 && sizes[(size_t)b] <= (int32_t)mmd::BLOCK_IN + 31, MM_ERR_DEVICE, "mm_bgzf_deflate: a member's size is out of range");
      offs[(size_t)b] = o; o += sizes[(size_t)b];
    }
    MM_REQUIRE(o <= out_cap, MM_ERR_DEVICE, "mm_bgzf_deflate: the members exceed the bound");
    par(nthr, [&](size_t t) {                                    // the members back to back into the caller's buffer
      for (size_t b = (size_t)n * t / nthr; b < (size_t)n * (t + 1) / nthr; ++b) memcpy(out + offs[b], down + b * mmd::MEMBER_MAX, (size_t)sizes[b]);
    });
  }
  *out_bytes = o;
  *n_blocks = (int32_t)nb;
}

}  // namespace mm
