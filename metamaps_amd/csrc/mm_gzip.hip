// Plain gzip inflated on the device (mm_gzip_open / feed / read): the device backend of mm_gzip.hpp's driver.  DESIGN.md §1 ("Plain gzip on
// the device") has the shape and what it costs.
//
//   gz_jobs_kernel     one wavefront per chunk: find a block start (lane-parallel test of 64 bit offsets at a time, then a trial decode),
//                      decode speculatively with a window of markers into the chunk's slot in HBM (16-bit entries: a byte, or a marker).
//                      The same kernel, with one job, decodes a chunk again from a known position with the known window.
//   gz_win_kernel      the carried 32 KiB window into a slot's window region, or out of a slot's resolved tail (one step of the walk).
//   gz_resolve_kernel  one workgroup per piece: markers replaced by their bytes, the bytes written out, the piece's CRC32 across the threads.
//
// LDS of gz_jobs_kernel: the Huffman tables and code lengths (~6 KiB), the constant tables (~1.4 KiB) and the 4 KiB input ring: ~12 KiB.
// The output and its window stay in HBM (a slot is WIN + cap entries), so occupancy is set by registers, not by LDS.
#include "mm_codec.hpp"
#include "mm_gzip.hpp"
#include "mm_wave_lanes.hpp"
#include <algorithm>

namespace {

__constant__ mmi::Consts k_gz_consts = mmi::make_consts();

__device__ void load_consts(mmi::Consts& K) {
  static_assert(sizeof(mmi::Consts) % 4 == 0, "");
  const uint32_t* src = (const uint32_t*)&k_gz_consts;
  uint32_t* dst = (uint32_t*)&K;
  for (uint32_t i = threadIdx.x; i < sizeof(mmi::Consts) / 4; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

__global__ __launch_bounds__(64) void gz_jobs_kernel(const uint8_t* __restrict__ in, uint32_t n, const mmg::Job* __restrict__ jobs,
                                                     mmg::Res* __restrict__ res, uint16_t* slots, uint64_t stride, uint32_t cap) {
  __shared__ mmi::Consts K;
  __shared__ mmi::Scratch S;
  __shared__ uint8_t ring[mmi::RING];
  load_consts(K);
  mmi::WaveLanes p;
  p.ring = ring;
  const mmg::Job j = jobs[blockIdx.x];
  mmg::Res r;
  mmg::gz_run_job(p, S, K, in, n, slots + j.slot * stride, cap, j, r);
  if (threadIdx.x == 0) res[blockIdx.x] = r;
}

// to_slot: slot[0, WIN) := W.  Otherwise W := the resolved entries [len, len + WIN) of the slot (its last WIN of [0, WIN + len)).
__global__ __launch_bounds__(256) void gz_win_kernel(uint16_t* W, uint16_t* slot, uint32_t len, int to_slot) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= mmg::WIN) return;
  if (to_slot) slot[t] = W[t];
  else W[t] = mmg::resolve_entry(slot, len + t);
}

struct DevPiece { uint64_t slot_off, out_off; uint32_t len, pad; };

__global__ __launch_bounds__(256) void gz_resolve_kernel(const uint16_t* __restrict__ slots, const DevPiece* __restrict__ pieces,
                                                         uint8_t* __restrict__ out, uint32_t* __restrict__ crc, int64_t* __restrict__ bad) {
  __shared__ mmi::Consts K;
  __shared__ int first_bad;
  __shared__ uint32_t x[8];
  load_consts(K);
  const DevPiece pc = pieces[blockIdx.x];
  const uint16_t* w = slots + pc.slot_off;
  uint8_t* o = out + pc.out_off;
  const uint32_t n = pc.len, T = blockDim.x, t = threadIdx.x;
  if (t == 0) first_bad = INT32_MAX;
  __syncthreads();
  int my_bad = INT32_MAX;
  for (uint32_t i = t; i < n; i += T) {
    const uint16_t v = mmg::resolve_entry(w, mmg::WIN + i);
    if (v == mmg::INVALID && my_bad == INT32_MAX) my_bad = (int)i;
    o[i] = (uint8_t)v;
  }
  if (my_bad != INT32_MAX) atomicMin(&first_bad, my_bad);
  __syncthreads();                                               // (the piece's bytes are written before the threads read them back)
  // CRC32 of o[0, n): thread t's contiguous part, shifted over the bytes behind it, XORed together (mm_inflate.hpp crc32_lanes)
  const uint32_t part = (n + T - 1) / T;
  const uint32_t lo = std::min(n, t * part), hi = std::min(n, lo + part);
  uint32_t c = 0;
  for (uint32_t i = lo; i < hi; ++i) c = K.crc.byte[(c ^ o[i]) & 255] ^ (c >> 8);
  uint32_t v = hi > lo ? mmi::crc_multmodp(mmi::crc_shift_bytes(K.crc, n - hi), c) : 0;
  if (t == 0) v ^= mmi::crc_multmodp(mmi::crc_shift_bytes(K.crc, n), 0xFFFFFFFFu);
#pragma unroll
  for (int s = 32; s; s >>= 1) v ^= (uint32_t)__shfl_xor((int)v, s, 64);
  if ((t & 63) == 0) x[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    uint32_t a = 0;
    for (uint32_t k = 0; k < (T + 63) / 64; ++k) a ^= x[k];
    crc[blockIdx.x] = ~a;
    bad[blockIdx.x] = first_bad == INT32_MAX ? -1 : first_bad;
  }
}

}  // namespace

namespace mm {

// mmg::Stream's device backend: the round's input, the slots and the carried window in HBM of the context's device
struct GzipDevice {
  mm_ctx* ctx;
  DBuf<uint8_t> d_in, d_out;
  DBuf<uint16_t> d_slots, d_W;
  DBuf<mmg::Job> d_jobs;
  DBuf<mmg::Res> d_res;
  DBuf<DevPiece> d_pieces;
  DBuf<uint32_t> d_crc;
  DBuf<int64_t> d_bad;
  uint32_t cap = 0, n_in = 0;
  explicit GzipDevice(mm_ctx* c) : ctx(c) {}
  hipStream_t st() const { return ctx->stream; }
  uint64_t stride() const { return (uint64_t)mmg::WIN + cap; }
  template <class T> static void want(DBuf<T>& b, size_t n) { if (b.n < n) b.alloc(std::max<size_t>(n, b.n + b.n / 4)); }
  void begin_round(const uint8_t* in, uint32_t n, uint32_t nslots, uint32_t c) {
    cap = c; n_in = n;
    want(d_in, std::max<uint32_t>(n, 1));
    d_in.upload(in, n, st());
    want(d_slots, (size_t)nslots * stride());
    if (!d_W.p) win_reset();
  }
  void run(const mmg::Job* jobs, uint32_t nj, mmg::Res* res) {
    want(d_jobs, nj); want(d_res, nj);
    d_jobs.upload(jobs, nj, st());
    gz_jobs_kernel<<<dim3(nj), dim3(64), 0, st()>>>(d_in.p, n_in, d_jobs.p, d_res.p, d_slots.p, stride(), cap);
    MM_KERNEL_CHECK();
    d_res.download(res, nj, st());
    MM_HIP(mm::stream_sync(st()));
  }
  void win_reset() {
    want(d_W, mmg::WIN);
    MM_HIP(hipMemsetAsync(d_W.p, 0xFF, mmg::WIN * sizeof(uint16_t), st()));
  }
  void win_to_slot(uint32_t s) {
    gz_win_kernel<<<dim3(mmg::WIN / 256), dim3(256), 0, st()>>>(d_W.p, d_slots.p + s * stride(), 0, 1);
    MM_KERNEL_CHECK();
  }
  void win_from_slot(uint32_t s, uint32_t len) {
    gz_win_kernel<<<dim3(mmg::WIN / 256), dim3(256), 0, st()>>>(d_W.p, d_slots.p + s * stride(), len, 0);
    MM_KERNEL_CHECK();
  }
  void resolve(const mmg::Piece* pc, uint32_t np, uint8_t* dst, uint32_t* crc, int64_t* bad) {
    std::vector<DevPiece> dp(np);
    uint64_t total = 0;
    for (uint32_t i = 0; i < np; ++i) { dp[i] = DevPiece{pc[i].slot * stride(), total, pc[i].len, 0}; total += pc[i].len; }
    want(d_pieces, np); want(d_crc, np); want(d_bad, np); want(d_out, std::max<uint64_t>(total, 1));
    d_pieces.upload(dp.data(), np, st());
    gz_resolve_kernel<<<dim3(np), dim3(256), 0, st()>>>(d_slots.p, d_pieces.p, d_out.p, d_crc.p, d_bad.p);
    MM_KERNEL_CHECK();
    d_crc.download(crc, np, st());
    d_bad.download(bad, np, st());
    if (total) {
      uint8_t* const down = (uint8_t*)ctx->pinned_at_least((size_t)total);
      d_out.download(down, (size_t)total, st());
      MM_HIP(mm::stream_sync(st()));
      // the pinned bytes to the caller's on up to 16 threads, as mm_bgzf_inflate copies large batches
      const size_t nthr = (size_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)std::max(1u, mm::cpu_budget() / 2), 16, (total >> 23) + 1}));
      if (nthr > 1) {
        if (!ctx->pack_pool) ctx->pack_pool = std::make_unique<TaskPool>(31);
        ctx->pack_pool->run(nthr, [&](size_t t) { const size_t a = total * t / nthr, b = total * (t + 1) / nthr; if (b > a) memcpy(dst + a, down + a, b - a); });
      } else {
        memcpy(dst, down, (size_t)total);
      }
    } else {
      MM_HIP(mm::stream_sync(st()));
    }
  }
};

}  // namespace mm

// the handle behind mm_gzip* (mm_api.hip)
struct mm_gzip {
  mm_ctx* ctx;
  mm::GzipDevice dev;
  mmg::Stream<mm::GzipDevice> z;
  size_t rd = 0;                                                 // bytes of z.out() already read
  mm_gzip(mm_ctx* c, uint64_t chunk, uint64_t segment) : ctx(c), dev(c), z(dev, chunk, segment) {}
};

namespace mm {

mm_gzip* gzip_open(mm_ctx* ctx, int64_t chunk, int64_t segment) {
  if (chunk <= 0) { const char* e = getenv("MM_GZIP_CHUNK_BYTES"); chunk = e ? std::max(256LL, atoll(e)) : (int64_t)mmg::DEFAULT_CHUNK; }
  if (segment <= 0) segment = (int64_t)mmg::Stream<GzipDevice>::DEFAULT_SEGMENT;
  return new mm_gzip(ctx, (uint64_t)chunk, (uint64_t)segment);
}
void gzip_close(mm_gzip* g) { delete g; }
mm_ctx* gzip_ctx(const mm_gzip* g) { return g->ctx; }
// 0, or -1 for corrupt data (the message names the compressed byte offset)
int gzip_feed(mm_gzip* g, const uint8_t* comp, int64_t n, bool last, int64_t* avail) {
  if (g->rd && g->rd == g->z.out().size()) { g->z.out().clear(); g->rd = 0; }
  const int rc = g->z.feed(comp, (size_t)n, last);
  if (avail) *avail = (int64_t)(g->z.out().size() - g->rd);
  if (rc) { g->ctx->err = "mm_gzip_feed: " + g->z.error(); return -1; }
  return 0;
}
int64_t gzip_read(mm_gzip* g, uint8_t* out, int64_t cap) {
  const size_t k = std::min<size_t>((size_t)cap, g->z.out().size() - g->rd);
  if (k) memcpy(out, g->z.out().data() + g->rd, k);
  g->rd += k;
  if (g->rd == g->z.out().size()) { g->z.out().clear(); g->rd = 0; }
  return (int64_t)k;
}
void gzip_stats(const mm_gzip* g, int64_t* counts, double* seconds) {
  const mmg::Stats& s = g->z.st;
  if (counts) { counts[0] = s.chunks; counts[1] = s.accepted; counts[2] = s.redone; counts[3] = s.skipped; counts[4] = (int64_t)g->z.members(); }
  if (seconds) { seconds[0] = s.t_spec; seconds[1] = s.t_chain; seconds[2] = s.t_resolve; seconds[3] = s.t_total; }
}

}  // namespace mm
