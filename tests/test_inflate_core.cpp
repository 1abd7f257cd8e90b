// CPU driver of the BGZF decode core (metamaps_amd/csrc/mm_inflate.hpp, one lane), driven by tests/test_inflate_core.py.
//   t IN OUT   IN: blocks, each a little-endian u32 length and that many bytes of one BGZF block.  For each block one line "status isize" on
//              stdout, and its inflated bytes (u32 length, bytes) appended to OUT when the status is ok.  Each block is copied into a buffer of
//              exactly its size and inflated into one of exactly its ISIZE, so a build with -fsanitize=address sees any access outside them.
#include "../metamaps_amd/csrc/mm_inflate.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: t IN OUT\n"); return 1; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open\n"); return 1; }
  static const mmi::Consts K = mmi::make_consts();
  auto S = std::make_unique<mmi::Scratch>();
  mmi::HostLanes p;
  for (;;) {
    uint8_t h[4];
    if (fread(h, 1, 4, in) != 4) break;
    const uint32_t n = mmi::rd32(h);
    std::unique_ptr<uint8_t[]> blk(new uint8_t[n ? n : 1]);
    if (n && fread(blk.get(), 1, n, in) != n) { fprintf(stderr, "short input\n"); return 1; }
    // the output buffer: exactly the ISIZE the trailer claims when it can be read and is in range, else none at all
    uint32_t cap = 0;
    if (n >= 26 && mmi::rd32(blk.get() + n - 4) <= mmi::MAX_ISIZE) cap = mmi::rd32(blk.get() + n - 4);
    std::unique_ptr<uint8_t[]> o(cap ? new uint8_t[cap] : nullptr);
    uint32_t isize = 0;
    const int32_t st = mmi::inflate_bgzf(p, *S, K, blk.get(), n, o.get(), &isize);
    printf("%d %u\n", st, isize);
    if (st == mmi::OK) {
      uint8_t l[4] = {(uint8_t)isize, (uint8_t)(isize >> 8), (uint8_t)(isize >> 16), (uint8_t)(isize >> 24)};
      fwrite(l, 1, 4, out);
      if (isize) fwrite(o.get(), 1, isize, out);
    }
  }
  fclose(out);
  fclose(in);
  return 0;
}
