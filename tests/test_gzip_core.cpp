// CPU driver of the plain gzip decoder (metamaps_amd/csrc/mm_gzip.hpp on the host backend, one lane), driven by tests/test_gzip_core.py.
//   t IN OUT CHUNK SEGMENT SEED   inflates the gzip stream IN with chunks of CHUNK and segments of SEGMENT compressed bytes, fed in pieces cut
//                                 at pseudo-random offsets (SEED 0: all at once; cN: a first piece of N bytes, then the rest), each piece
//                                 in a buffer of exactly its size.  stdout: one line
//                                 "rc offset chunks accepted redone skipped members", then the error text if rc != 0.  OUT: the inflated bytes.
#include "../metamaps_amd/csrc/mm_gzip.hpp"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: t IN OUT CHUNK SEGMENT SEED\n"); return 1; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "cannot open\n"); return 1; }
  std::vector<uint8_t> data;
  for (int c; (c = fgetc(in)) != EOF;) data.push_back((uint8_t)c);
  fclose(in);
  const uint64_t chunk = strtoull(argv[3], nullptr, 10), seg = strtoull(argv[4], nullptr, 10);
  const bool cut = argv[5][0] == 'c';
  const uint64_t first = cut ? strtoull(argv[5] + 1, nullptr, 10) : 0;
  uint64_t seed = cut ? 0 : strtoull(argv[5], nullptr, 10);
  auto be = std::make_unique<mmg::HostBackend>();
  mmg::Stream<mmg::HostBackend> z(*be, chunk, seg);
  int rc = 0;
  size_t at = 0;
  do {
    size_t n = data.size() - at;
    if (cut && at == 0) n = std::min<size_t>(n, first);
    if (seed && n) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; n = std::min<size_t>(n, 1 + (size_t)((seed >> 33) % (2 * seg + 1))); }
    std::unique_ptr<uint8_t[]> piece(new uint8_t[n ? n : 1]);
    if (n) memcpy(piece.get(), data.data() + at, n);
    at += n;
    rc = z.feed(piece.get(), n, at == data.size());
  } while (rc == 0 && at < data.size());
  printf("%d %llu %lld %lld %lld %lld %llu\n", rc, (unsigned long long)z.error_offset(), (long long)z.st.chunks, (long long)z.st.accepted,
         (long long)z.st.redone, (long long)z.st.skipped, (unsigned long long)z.members());
  if (rc) printf("%s\n", z.error().c_str());
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 1;
  if (!z.out().empty()) fwrite(z.out().data(), 1, z.out().size(), out);
  fclose(out);
  return 0;
}
