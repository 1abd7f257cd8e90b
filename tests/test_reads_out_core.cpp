// mm_reads_out_core.hpp on the host (tests/test_reads_out_core.py).  stdin: one record per line, `n_reads read with_qual name bases quals`, the last three in
// hex, `.` for no bytes, quals `-` for a read without qualities.  stdout per record: `R <rule>` for a refusal, else `B <size> <hex of the record>`.  The
// record is written into a buffer of exactly record_size bytes between guard bytes, and every byte is also asked of record_byte.
#include "../metamaps_amd/csrc/mm_reads_out_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "." || s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    long long n_reads, read; int with_qual; std::string name_h, bases_h, quals_h;
    if (!(is >> n_reads >> read >> with_qual >> name_h >> bases_h >> quals_h)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    const std::vector<uint8_t> name = unhex(name_h), bases = unhex(bases_h), quals = unhex(quals_h);
    const int rule = mmr::check(read, n_reads, (const char*)name.data(), (int64_t)name.size());
    if (rule) {
      const std::string t = mmr::rule_text(rule);
      if (t.rfind("rule " + std::to_string(rule) + ":", 0) != 0) { fprintf(stderr, "rule_text(%d) = %s\n", rule, t.c_str()); return 3; }
      printf("R %d\n", rule);
      continue;
    }
    if (quals_h != "-" && quals.size() != bases.size()) { fprintf(stderr, "qualities and bases differ in number\n"); return 2; }
    const int64_t m = (int64_t)bases.size(), l = (int64_t)name.size(), size = mmr::record_size(l, m, with_qual != 0);
    // heap copies of exactly the bytes that may be read: the address sanitizer sees any read beside them
    std::vector<uint8_t> b(bases), q(quals), nm(name);
    const mmr::QualBytes src{b.data(), quals_h == "-" ? nullptr : q.data()};
    std::vector<uint8_t> buf((size_t)size + 2, 0xA5);
    mmr::HostLanes p;
    const int64_t got = mmr::write_record(p, src, (const char*)nm.data(), l, m, with_qual != 0, buf.data() + 1);
    if (got != size || buf[0] != 0xA5 || buf[(size_t)size + 1] != 0xA5) { fprintf(stderr, "size or guard bytes\n"); return 4; }
    for (int64_t o = 0; o < size; ++o)
      if (mmr::record_byte(src, (const char*)nm.data(), l, m, with_qual != 0, o) != buf[(size_t)o + 1]) { fprintf(stderr, "record_byte(%lld)\n", (long long)o); return 5; }
    if (with_qual && (mmr::qual_at(l, m) + m + 1 != size || mmr::bases_at(l) + m + 3 != mmr::qual_at(l, m))) { fprintf(stderr, "layout\n"); return 6; }
    printf("B %lld ", (long long)size);
    for (int64_t o = 0; o < size; ++o) printf("%02x", buf[(size_t)o + 1]);
    printf("\n");
  }
  return 0;
}
