// CPU harness: the sizing rules of the device allocator (metamaps_amd/csrc/mm_alloc_rules.hpp) against their formulas, restated here without the
// header's bit tricks, over powers of two +-1 from 1 byte to 256 GiB and <n> random sizes.  Prints "ok <n>" or the first fault.
#include "../metamaps_amd/csrc/mm_alloc_rules.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef unsigned long long u64;
static const u64 KiB = 1024, MiB = 1024 * KiB, GiB = 1024 * MiB;

static u64 pow2_below(u64 b) { u64 p = 1; while (p * 2 <= b) p *= 2; return p; }          // largest power of two <= b (b >= 1)
static u64 ceil_to(u64 b, u64 g) { return (b + g - 1) / g * g; }
// the formulas
static u64 ref_round_up(u64 b) { return b < 4096 ? 4096 : ceil_to(b, pow2_below(b) / 8); }
static bool ref_cache_fits(u64 have, u64 want) { return have >= want && have <= want + want / 4 + (want >= 256 * KiB ? want * 7 / 20 : 0); }
static u64 ref_ask(u64 want, bool roomy) {
  if (want >= 64 * MiB) return roomy ? ref_round_up(want + want / 4) : want;
  if (want >= 256 * KiB) return ref_round_up(want + want / 4);
  return want;
}
static u64 ref_class(u64 b) { u64 g = pow2_below(b < 1 ? 1 : b) / 64; if (g < 16 * MiB) g = 16 * MiB; return ceil_to(b, g); }
static bool ref_pool_fits(u64 have, u64 want) { return have >= want && have <= want + want / 8; }

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int check_size(u64 b) {
  const u64 r = mm::round_up(b), c = mm::index_scale_class(b);
  if (r != ref_round_up(b)) FAIL("round_up(%llu) = %llu, formula %llu", b, r, ref_round_up(b));
  if (r < b || r < 4096) FAIL("round_up(%llu) = %llu is too small", b, r);
  if (b >= 4096 && (r - b) * 8 > b) FAIL("round_up(%llu) = %llu: more than 12.5 %% slack", b, r);
  if (mm::round_up(r) != r) FAIL("round_up is not idempotent at %llu", b);
  if (c != ref_class(b)) FAIL("index_scale_class(%llu) = %llu, formula %llu", b, c, ref_class(b));
  if (c < b || c % (16 * MiB)) FAIL("index_scale_class(%llu) = %llu: below the request or off the 16 MiB granule", b, c);
  if (c - b >= 16 * MiB && (c - b) * 1000 > b * 16) FAIL("index_scale_class(%llu) = %llu: more than a granule and more than 1.6 %% slack", b, c);
  if (mm::index_scale_class(c) != c) FAIL("index_scale_class is not idempotent at %llu", b);
  for (int roomy = 0; roomy < 2; ++roomy) {
    const u64 a = mm::ask_bytes(r, roomy);
    if (a != ref_ask(r, roomy)) FAIL("ask_bytes(%llu, %d) = %llu, formula %llu", r, roomy, a, ref_ask(r, roomy));
    if (a < r) FAIL("ask_bytes(%llu, %d) = %llu is below the request", r, roomy, a);
    if (!mm::cache_fits(a, r)) FAIL("a block of %llu bytes, asked for a request of %llu, would not serve that request from the cache", a, r);
  }
  // the two fit rules around their edges, and a step beyond
  const u64 edge_c = r + r / 4 + (r >= 256 * KiB ? r * 7 / 20 : 0), edge_p = b + b / 8;
  const u64 haves[] = {b, r, r + 1, edge_c - 1, edge_c, edge_c + 1, edge_p - 1, edge_p, edge_p + 1, 2 * r, r - 1, b > 0 ? b - 1 : 0};
  for (u64 h : haves) {
    if (mm::cache_fits(h, r) != ref_cache_fits(h, r)) FAIL("cache_fits(%llu, %llu) = %d", h, r, (int)mm::cache_fits(h, r));
    if (mm::pool_block_fits(h, b) != ref_pool_fits(h, b)) FAIL("pool_block_fits(%llu, %llu) = %d", h, b, (int)mm::pool_block_fits(h, b));
  }
  return 0;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  if (mm::SLAB_FROM_BYTES != 1 * MiB) FAIL("SLAB_FROM_BYTES = %zu", mm::SLAB_FROM_BYTES);
  if (mm::device_roomy(20, 100) || !mm::device_roomy(21, 100) || mm::device_roomy(0, 0)) FAIL("device_roomy: headroom while more than a fifth is free");
  std::vector<u64> sizes;
  for (int lg = 0; lg <= 38; ++lg) for (int d = -1; d <= 1; ++d) { const u64 b = ((u64)1 << lg) + d; if (b >= 1) sizes.push_back(b); }
  std::mt19937_64 rng(7);
  for (long i = 0; i < n; ++i) { const int lg = (int)(rng() % 39); sizes.push_back(((u64)1 << lg) + rng() % ((u64)1 << lg)); }   // (every power of two's range alike)
  for (u64 b : sizes) if (check_size(b)) return 1;
  // monotone: a larger request never gets a smaller block
  std::sort(sizes.begin(), sizes.end());
  for (size_t i = 1; i < sizes.size(); ++i) {
    const u64 a = sizes[i - 1], b = sizes[i];
    if (mm::round_up(a) > mm::round_up(b)) FAIL("round_up is not monotone between %llu and %llu", a, b);
    if (mm::index_scale_class(a) > mm::index_scale_class(b)) FAIL("index_scale_class is not monotone between %llu and %llu", a, b);
    for (int roomy = 0; roomy < 2; ++roomy)
      if (mm::ask_bytes(mm::round_up(a), roomy) > mm::ask_bytes(mm::round_up(b), roomy) && ((mm::round_up(a) >= 64 * MiB) == (mm::round_up(b) >= 64 * MiB)))
        FAIL("ask_bytes is not monotone between %llu and %llu", a, b);
  }
  printf("ok %zu sizes\n", sizes.size());
  return 0;
}
