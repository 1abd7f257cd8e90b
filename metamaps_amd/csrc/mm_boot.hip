// Read-level Poisson bootstrap of the EM (not in the reference; DESIGN.md section 4, "Bootstrap"): replicates of the weighted EM
//   S_r(i)   = sum over the mappings m of read i of f_r[t_m] * inv_nloc_m * mapq_m                      (fEM.h:350-361)
//   sum_r[t] = sum_i w(r, i) * sum over the mappings of i on t of f_r[t] * inv_nloc_m * mapq_m / S_r(i)
//   f_r     <- sum_r / sum_t sum_r[t]                                                               (fEM.h:606-615)
//   ll_r     = sum_i w(r, i) * log S_r(i)                                                           (fEM.h:578)
// with the reference's stop rule per replicate (fEM.h:624-639); a replicate that has stopped is frozen.  The weights come from
// mm_boot_core.hpp (or from the caller) and are never stored.  A replicate whose weighted sample is empty has no estimate: f_r = 0, ll_r = 0,
// no iterations, stopped (P3b sees a total of exactly 0 in its first iteration and freezes it).
//
// The loop is the point EM's (mm_post.hip: P1 | P2 | P3 per iteration, enqueued in groups with one read of the control words behind each)
// with a replicate dimension.  A tile is 64 replicates, one per lane of a wavefront:
//   P1b  workgroup = the point EM's block of reads x one tile; four rows of lanes walk the block's reads.  A mapping's taxon / inv_nloc /
//        mapq / pos are loaded once per row and serve the tile's 64 replicates; f is kept [taxon][replicate], so the 64 values of one
//        taxon are one contiguous load.  One reciprocal of S_r(i) per (read, replicate).  The weighted posterior goes to
//        post_b[pos(m) * B + r] (taxon-sorted, replicate-minor); per workgroup and replicate the sum of w * log S.
//   P2b  workgroup = one item of the point EM's per-taxon sums (<= 512 consecutive entries of one taxon) x one tile: lanes over
//        (entry row, replicate), each load of a wavefront is 64 consecutive doubles.
//   P3b  workgroup = one tile: per replicate the per-taxon sums, their total, f_r, ll_r and the stop rule.
// Every sum has a fixed shape that depends on neither the number of replicates of the call nor their tiling (the tile width and the rows are
// constants): results are bit-identical from run to run and for any split of the replicates over calls or devices.  No floating-point atomics.
// The communicator of the context, if any, is never used: the replicates are split over devices instead.
#include "mm_em.hpp"
#include "mm_boot_core.hpp"
#include <algorithm>

namespace mm {

constexpr int BOOT_RT = 64;                                       // replicates per tile (lanes of a wavefront)
constexpr int BOOT_P1_ROWS = 4, BOOT_P2_ROWS = 4, BOOT_P3_ROWS = 16;

struct BootLoop {
  const int64_t* read_off; const int32_t* mread;                  // [n_reads + 1]; index of a read among the mapped reads
  const int32_t* taxon; const double* mapq; const double* inv_nloc; const int64_t* pos;
  int64_t n_reads, n_mapped;
  const int64_t* item_lo; const int64_t* item_hi; int n_items;
  const int32_t* present; const int32_t* pt_item; int n_present;
  double* post_b;                                                 // [n_entries][B], taxon-sorted
  double* item_b;                                                 // [n_items][B]
  double* wg_ll_b;                                                // [n_wg][B]
  double* tsum_b;                                                 // [n_present][B]
  double* f_b;                                                    // [n_taxa][B] (rows of present taxa only)
  long long* ctrl_b;                                              // [B][4]: iterations done, stopped (1: rule, 2: limit, 3: empty sample), bits of the previous ll, 0
  int B, rep0; uint64_t seed; const uint8_t* weights;             // weights: [B][n_mapped] from the caller, or nullptr: boot_weight
  long long it_limit;
};

__device__ inline bool boot_live(const BootLoop& a, int rep) { return rep < a.B && a.ctrl_b[(int64_t)rep * 4 + 1] == 0; }

__global__ void __launch_bounds__(256) boot_p1_kernel(BootLoop a) {
  __shared__ double sh[256];
  const int tid = threadIdx.x, rr = tid % BOOT_RT, row = tid / BOOT_RT;
  const int rep = blockIdx.y * BOOT_RT + rr;
  const bool on = boot_live(a, rep);
  if (!__syncthreads_or(on)) return;
  const int64_t n_wg = gridDim.x, B = a.B;
  const int64_t rb = (a.n_reads + n_wg - 1) / n_wg, R0 = min((int64_t)blockIdx.x * rb, a.n_reads), R1 = min(R0 + rb, a.n_reads);
  double ll = 0;
  if (on) {
    for (int64_t r = R0 + row; r < R1; r += BOOT_P1_ROWS) {
      const int64_t lo = a.read_off[r], hi = a.read_off[r + 1];
      if (hi <= lo) continue;
      const int64_t mi = a.mread[r];
      const int w = a.weights ? (int)a.weights[(int64_t)rep * a.n_mapped + mi] : boot_weight(a.seed, (uint32_t)(a.rep0 + rep), (uint32_t)mi);
      if (w == 0) {                                               // the read is not in this replicate: its posteriors count 0
        for (int64_t i = lo; i < hi; ++i) a.post_b[a.pos[i] * B + rep] = 0.0;
        continue;
      }
      const int64_t last = hi - 1;
      double sum = 0, l8[8]; int64_t p8[8];
      for (int64_t c = lo; c < hi; c += 8) {                      // eight mappings' loads in flight before the first is used (clamped, no branches)
        int t8[8]; double w8[8], q8[8], f8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int64_t i = c + u < last ? c + u : last; t8[u] = a.taxon[i]; w8[u] = a.inv_nloc[i]; q8[u] = a.mapq[i]; p8[u] = a.pos[i]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) f8[u] = a.f_b[(int64_t)t8[u] * B + rep];
#pragma unroll
        for (int u = 0; u < 8; ++u) { l8[u] = f8[u] * w8[u] * q8[u]; if (c + u < hi) sum += l8[u]; }   // fEM.h:353, in mapping order
      }
      const double wd = (double)w, ws = wd / sum;                 // one reciprocal per (read, replicate)
      if (hi - lo <= 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) if (lo + u < hi) a.post_b[p8[u] * B + rep] = l8[u] * ws;
      } else {                                                    // a long read: its likelihoods once more (the loads hit the cache)
        for (int64_t c = lo; c < hi; c += 8) {
          int t8[8]; double w8[8], q8[8], f8[8]; int64_t q_pos[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) { const int64_t i = c + u < last ? c + u : last; t8[u] = a.taxon[i]; w8[u] = a.inv_nloc[i]; q8[u] = a.mapq[i]; q_pos[u] = a.pos[i]; }
#pragma unroll
          for (int u = 0; u < 8; ++u) f8[u] = a.f_b[(int64_t)t8[u] * B + rep];
#pragma unroll
          for (int u = 0; u < 8; ++u) if (c + u < hi) a.post_b[q_pos[u] * B + rep] = (f8[u] * w8[u] * q8[u]) * ws;
        }
      }
      ll += wd * log(sum);                                        // fEM.h:578
    }
  }
  sh[tid] = ll;
  __syncthreads();
  for (int d = 128; d >= BOOT_RT; d >>= 1) { if (tid < d) sh[tid] += sh[tid + d]; __syncthreads(); }
  if (row == 0 && on) a.wg_ll_b[(int64_t)blockIdx.x * B + rep] = sh[rr];
}

// one item (<= 512 entries of one taxon) x one tile: row k adds the entries k, k + 4, ... in order, the four rows are added in a fixed tree
__global__ void __launch_bounds__(256) boot_p2_kernel(BootLoop a) {
  __shared__ double sh[256];
  const int tid = threadIdx.x, rr = tid % BOOT_RT, row = tid / BOOT_RT;
  const int rep = blockIdx.y * BOOT_RT + rr;
  const bool on = boot_live(a, rep);
  if (!__syncthreads_or(on)) return;
  const int it = blockIdx.x;
  const int64_t B = a.B, lo = a.item_lo[it], hi = a.item_hi[it], last = hi - 1;
  double acc = 0;
  if (on) {
    for (int64_t j = lo + row; j < hi; j += 8 * BOOT_P2_ROWS) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int64_t e = j + u * BOOT_P2_ROWS; v[u] = a.post_b[(e < last ? e : last) * B + rep]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) if (j + u * BOOT_P2_ROWS < hi) acc += v[u];
    }
  }
  sh[tid] = acc;
  __syncthreads();
  for (int d = 128; d >= BOOT_RT; d >>= 1) { if (tid < d) sh[tid] += sh[tid + d]; __syncthreads(); }
  if (row == 0 && on) a.item_b[(int64_t)it * B + rep] = sh[rr];
}

// one tile: 16 rows of lanes share the present taxa and the P1b partials; fixed trees over the rows
__global__ void __launch_bounds__(1024) boot_p3_kernel(BootLoop a, int n_wg) {
  __shared__ double sh_t[1024], sh_l[1024];
  const int tid = threadIdx.x, rr = tid % BOOT_RT, row = tid / BOOT_RT;
  const int rep = blockIdx.x * BOOT_RT + rr;
  const bool on = boot_live(a, rep);
  if (!__syncthreads_or(on)) return;
  const int64_t B = a.B;
  double tot = 0, ll = 0;
  if (on) {
    for (int p = row; p < a.n_present; p += BOOT_P3_ROWS) {       // the item sums of a taxon in order (P3 of the point EM)
      const int i0 = a.pt_item[p], i1 = a.pt_item[p + 1];
      double s = 0;
      for (int it = i0; it < i1; it += 4) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = a.item_b[(int64_t)min(it + u, i1 - 1) * B + rep];
#pragma unroll
        for (int u = 0; u < 4; ++u) if (it + u < i1) s += v[u];
      }
      a.tsum_b[(int64_t)p * B + rep] = s;
      tot += s;
    }
    for (int g = row; g < n_wg; g += BOOT_P3_ROWS) ll += a.wg_ll_b[(int64_t)g * B + rep];
  }
  sh_t[tid] = tot; sh_l[tid] = ll;
  __syncthreads();
  for (int d = 512; d >= BOOT_RT; d >>= 1) { if (tid < d) { sh_t[tid] += sh_t[tid + d]; sh_l[tid] += sh_l[tid + d]; } __syncthreads(); }
  const double total = sh_t[rr], llr = sh_l[rr];
  if (!on) return;
  // A replicate that drew no read (every mapped read at weight 0, or a problem without mappings): every posterior is exactly 0, so total == 0
  // in its first iteration, and only then (a read of weight w adds posteriors that sum to w).  fEM.h:606-615 would divide 0 by 0: f_r = 0,
  // ll_r = 0, no iteration counted, frozen.
  const bool empty = total == 0;
  for (int p = row; p < a.n_present; p += BOOT_P3_ROWS) a.f_b[(int64_t)a.present[p] * B + rep] = empty ? 0.0 : a.tsum_b[(int64_t)p * B + rep] / total;   // fEM.h:606-615
  if (row == 0) {                                                 // the stop rule of this replicate (fEM.h:624-639), as em_stop_rule
    long long* c = a.ctrl_b + (int64_t)rep * 4;
    const long long it = c[0];
    if (empty && it == 0) { c[2] = 0; c[1] = 3; return; }
    const double ll_prev = __longlong_as_double(c[2]);
    long long stop = 0;
    if (it > 0 && (llr - ll_prev) <= 1 && (1 - llr / ll_prev) < 0.0001) stop = 1;
    else if (it + 1 >= a.it_limit) stop = 2;
    c[2] = __double_as_longlong(llr);
    c[0] = it + 1;
    c[1] = stop;
  }
}

__global__ void __launch_bounds__(256) boot_fill_kernel(const double* __restrict__ f0, const int32_t* __restrict__ present, int n_present, int B, double* __restrict__ f_b) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;      // f_b[t][r] = f0[t] for the present taxa
  if (k >= (int64_t)n_present * B) return;
  const int t = present[k / B];
  f_b[(int64_t)t * B + k % B] = f0[t];
}

int boot_run(mm_em* E, const double* f_start, int32_t rep0, int32_t n_rep, uint64_t seed, const uint8_t* weights, int max_iter,
             double* f_out, double* ll_out, int32_t* n_iter, int32_t* stopped) {
  hipStream_t st = E->ctx->stream;
  const int32_t T = E->n_taxa;
  const int64_t B = n_rep, ne = E->n_entries;
  // what the replicates need on the device, checked before anything is built: post_b dominates (n_entries * B * 8 bytes)
  MM_REQUIRE(ne <= ((int64_t)1 << 62) / 8 / B, MM_ERR_LIMIT, "bootstrap: n_entries * n_rep * 8 bytes overflow");
  MM_REQUIRE(ceil_div(B, BOOT_RT) <= 65535, MM_ERR_LIMIT, "bootstrap: more than 65535 * 64 replicates in one call");
  {
    size_t fr = 0, tot = 0;
    MM_HIP(dev_mem_info(&fr, &tot));
    const double need = 8.0 * (double)B * ((double)std::max<int64_t>(ne, 1) + (double)T);
    MM_REQUIRE(need <= (double)tot, MM_ERR_LIMIT, "bootstrap: " + std::to_string((long long)need) + " bytes of per-replicate buffers exceed the device's " +
                                                  std::to_string(tot) + " (tile the replicates)");
  }
  em_prepare(E);
  if (E->n_mapped < 0) {                                          // the reads' indices among the mapped reads (the weights' read index)
    std::vector<int64_t> ro = E->read_off.to_host(st, (size_t)E->n_reads + 1);
    std::vector<int32_t> mr((size_t)std::max<int64_t>(E->n_reads, 1), -1);
    int32_t k = 0;
    for (int64_t r = 0; r < E->n_reads; ++r) if (ro[(size_t)r + 1] > ro[(size_t)r]) mr[(size_t)r] = k++;
    E->mread.alloc(mr.size()); E->mread.upload(mr.data(), mr.size(), st);
    MM_HIP(mm::stream_sync(st));
    E->n_mapped = k;
  }
  const int n_tiles = (int)ceil_div(B, BOOT_RT);
  DBuf<double> post_b((size_t)std::max<int64_t>(ne, 1) * (size_t)B), item_b((size_t)std::max(E->n_items, 1) * (size_t)B),
      wg_ll_b((size_t)E->n_wg * (size_t)B), tsum_b((size_t)std::max(E->n_present, 1) * (size_t)B), f_b((size_t)T * (size_t)B), f0((size_t)T);
  DBuf<long long> ctrl_b((size_t)B * 4);
  DBuf<uint8_t> w_dev;
  if (weights) { w_dev.alloc((size_t)std::max<int64_t>(E->n_mapped * B, 1)); w_dev.upload(weights, (size_t)(E->n_mapped * B), st); }
  f_b.zero(st);
  f0.upload(f_start, (size_t)T, st);
  ctrl_b.zero(st);
  if (E->n_present > 0) {
    boot_fill_kernel<<<dim3((unsigned)ceil_div((int64_t)E->n_present * B, 256)), dim3(256), 0, st>>>(f0.p, E->present.p, E->n_present, (int)B, f_b.p);
    MM_KERNEL_CHECK();
  }
  BootLoop a{E->read_off.p, E->mread.p, E->taxon.p, E->mapq.p, E->inv_nloc.p, E->pos.p, E->n_reads, E->n_mapped,
             E->item_lo.p, E->item_hi.p, E->n_items, E->present.p, E->pt_item.p, E->n_present,
             post_b.p, item_b.p, wg_ll_b.p, tsum_b.p, f_b.p, ctrl_b.p, (int)B, rep0, seed, weights ? w_dev.p : nullptr, (long long)max_iter};
  std::vector<long long> h((size_t)B * 4, 0);
  // groups of iterations with one read of the control words behind each (em_run: a first group of 24, then eights); iterations of a replicate
  // that has stopped are no-ops, a tile whose replicates have all stopped leaves at once
  long long done = 0;
  for (int group_no = 0; done < max_iter; ++group_no) {
    const int g_n = (int)std::min<long long>(group_no == 0 ? 24 : 8, max_iter - done);
    for (int g = 0; g < g_n; ++g) {
      boot_p1_kernel<<<dim3((unsigned)E->n_wg, (unsigned)n_tiles), dim3(256), 0, st>>>(a); MM_KERNEL_CHECK();
      if (E->n_items > 0) { boot_p2_kernel<<<dim3((unsigned)E->n_items, (unsigned)n_tiles), dim3(256), 0, st>>>(a); MM_KERNEL_CHECK(); }
      boot_p3_kernel<<<dim3((unsigned)n_tiles), dim3(1024), 0, st>>>(a, E->n_wg); MM_KERNEL_CHECK();
    }
    done += g_n;
    ctrl_b.download(h.data(), h.size(), st);
    MM_HIP(mm::stream_sync(st));
    bool live = false;
    for (int64_t r = 0; r < B && !live; ++r) live = h[(size_t)r * 4 + 1] == 0;
    if (!live) break;
  }
  std::vector<double> fh = f_b.to_host(st, (size_t)T * (size_t)B);
  std::vector<char> pres((size_t)T, 0);
  { std::vector<int32_t> pr = E->present.to_host(st, (size_t)E->n_present); for (int32_t t : pr) pres[(size_t)t] = 1; }
  for (int64_t r = 0; r < B; ++r) {
    if (f_out) for (int32_t t = 0; t < T; ++t) f_out[r * T + t] = pres[(size_t)t] ? fh[(size_t)t * B + r] : 0.0;   // taxa without a mapping: 0 from the first iteration on
    long long bits = h[(size_t)r * 4 + 2];
    double ll; memcpy(&ll, &bits, sizeof ll);
    if (ll_out) ll_out[r] = ll;
    if (n_iter) n_iter[r] = (int32_t)h[(size_t)r * 4];
    if (stopped) stopped[r] = h[(size_t)r * 4 + 1] == 1 || h[(size_t)r * 4 + 1] == 3 ? 1 : 0;   // (3: an empty sample, n_iter == 0)
  }
  return 0;
}

}  // namespace mm
