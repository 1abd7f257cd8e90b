// Host driver of the BGZF deflate core (metamaps_amd/csrc/mm_deflate.hpp built with plain g++; tests/test_deflate_core.py drives it).
//   test_deflate_core IN OUT    IN is cut into blocks of 65 280 bytes and every block deflated into one BGZF member; the members go back to
//                               back into OUT.  One line per member on stdout: "<member bytes> <stored 0/1> <status>", status being what
//                               the project's own inflate core (mm_inflate.hpp) says about the member (0 ok) — 9 if its bytes differ from
//                               the input.  The member's destination and the token buffer are heap blocks of exactly the documented size,
//                               so the sanitizer build fails on a write outside them.
#include "../metamaps_amd/csrc/mm_deflate.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> in;
  uint8_t buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + n);
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  static const mmi::Consts K = mmi::make_consts();
  auto S = std::make_unique<mmd::Scratch>();
  auto IS = std::make_unique<mmi::Scratch>();
  mmd::HostLanes p;
  mmi::HostLanes ip;
  int64_t total = 0;
  for (size_t at = 0; at < in.size(); at += mmd::BLOCK_IN) {
    const uint32_t n = (uint32_t)std::min<size_t>(mmd::BLOCK_IN, in.size() - at);
    memcpy(S->in, in.data() + at, n);
    memset(S->in + n, 0, 16);
    std::unique_ptr<uint32_t[]> tok(new uint32_t[mmd::TOK_CAP]);
    uint8_t* dst = (uint8_t*)aligned_alloc(16, mmd::MEMBER_MAX);
    uint32_t stored = 0;
    const uint32_t m = mmd::deflate_member(p, *S, K, n, tok.get(), dst, &stored);
    std::vector<uint8_t> member(dst, dst + m), back(mmi::MAX_ISIZE);   // (exact-size copy for the inflate core's bounds)
    free(dst);
    uint32_t isize = 0;
    int st = mmi::inflate_bgzf(ip, *IS, K, member.data(), m, back.data(), &isize);
    if (st == 0 && (isize != n || memcmp(back.data(), in.data() + at, n) != 0)) st = 9;
    printf("%u %u %d\n", m, stored, st);
    fwrite(member.data(), 1, m, o);
    total += m;
  }
  fclose(o);
  if (total > mmd::bound((int64_t)in.size())) { fprintf(stderr, "bound exceeded\n"); return 1; }
  return 0;
}
