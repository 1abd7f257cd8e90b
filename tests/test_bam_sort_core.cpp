// The host's run of metamaps_amd/csrc/mm_bam_sort_core.hpp for tests/test_bam_sort_core.py: the steps of mm_bam_sort.hip with one lane and the standard
// library's sort and loops where the device has rocprim's, over the same definitions.
//   stdin   n_ref header_bytes window_bytes n_runs; per run: n_records, then per record ref pos end size, then the run's inflated bytes in hex ("-": none);
//           n_members, then every member's compressed size
//   stdout  the gathered stream in hex ("-": empty); the .bai in hex
// Every buffer a copy reads or writes has exactly the bytes the header promises (16 behind the last), so the sanitizers see any step outside.
#include "../metamaps_amd/csrc/mm_bam_sort_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <string>

struct Buf {                                                       // n bytes on a 16-byte boundary and 16 behind them, nothing more
  uint8_t* p = nullptr; explicit Buf(size_t n) { void* q = nullptr; if (posix_memalign(&q, 16, n + 16)) abort(); p = (uint8_t*)q; }
  ~Buf() { free(p); }
};
static void hex_out(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s; s.reserve(2 * n + 1);
  for (size_t i = 0; i < n; ++i) { s.push_back(d[p[i] >> 4]); s.push_back(d[p[i] & 15]); }
  puts(n ? s.c_str() : "-");
}

int main() {
  int32_t n_ref; int64_t header_bytes, window, n_runs;
  std::cin >> n_ref >> header_bytes >> window >> n_runs;
  std::vector<int32_t> ref, pos, end, run_of; std::vector<int64_t> src_off, size; std::vector<Buf*> raw;
  for (int64_t r = 0; r < n_runs; ++r) {
    int64_t n, at = 0; std::cin >> n;
    for (int64_t i = 0; i < n; ++i) {
      int32_t a, b, c; int64_t s; std::cin >> a >> b >> c >> s;
      ref.push_back(a); pos.push_back(b); end.push_back(c); run_of.push_back((int32_t)r); src_off.push_back(at); size.push_back(s); at += s;
    }
    std::string h; std::cin >> h;
    if (h == "-") h.clear();
    if ((int64_t)h.size() != 2 * at) return 2;
    raw.push_back(new Buf((size_t)at));
    for (int64_t i = 0; i < at; ++i) raw.back()->p[i] = (uint8_t)std::stoi(h.substr(2 * (size_t)i, 2), nullptr, 16);
  }
  int64_t n_mem; std::cin >> n_mem;
  std::vector<int64_t> member_at(1, header_bytes);
  for (int64_t m = 0; m < n_mem; ++m) { int64_t b; std::cin >> b; member_at.push_back(member_at.back() + b); }
  const int64_t n = (int64_t)ref.size();

  // plan: the stable sort by sort_key, the offsets
  std::vector<int64_t> perm((size_t)n), out_off((size_t)n + 1, 0);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return mmbs::sort_key(ref[a], pos[a]) < mmbs::sort_key(ref[b], pos[b]); });
  for (int64_t i = 0; i < n; ++i) out_off[i + 1] = out_off[i] + size[perm[i]];
  const int64_t total = out_off[n];
  if (mmbs::n_members(total) != n_mem) return 3;

  // windows: the gather kernel's loop per SPAN, one lane
  mmb::HostLanes lanes;
  std::vector<uint8_t> stream;
  for (int64_t lo = 0; lo < total; lo += window) {
    const int64_t hi = std::min(total, lo + window);
    Buf out((size_t)(hi - lo));
    for (int64_t c_lo = lo; c_lo < hi; c_lo += mmbs::SPAN) {
      const int64_t c_hi = std::min(hi, c_lo + mmbs::SPAN);
      for (int64_t i = mmbs::upper_record(out_off.data(), n, c_lo); i < n && out_off[i] < c_hi; ++i) {
        const int64_t g = perm[i];
        const mmbs::Piece pc = mmbs::clip(out_off[i], out_off[i + 1] - out_off[i], src_off[g], c_lo, c_hi);
        mmbs::copy_bytes(lanes, raw[run_of[g]]->p + pc.src, out.p + (c_lo - lo) + pc.dst, pc.len);
      }
    }
    stream.insert(stream.end(), out.p, out.p + (hi - lo));
  }
  hex_out(stream.data(), stream.size());

  // index: the records' offsets and keys in file order, the chunks, the linear index
  std::vector<uint64_t> vs((size_t)n), ve((size_t)n), bkey((size_t)n), M((size_t)n), ckey, cvs, cve, ioff, first_vs((size_t)n_ref, 0), last_ve((size_t)n_ref, 0);
  std::vector<int64_t> ord((size_t)n), ref_start((size_t)n_ref + 1, 0), win_off((size_t)n_ref + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t g = perm[i];
    vs[i] = mmbs::voff(out_off[i], member_at.data(), total); ve[i] = mmbs::voff(out_off[i + 1], member_at.data(), total);
    bkey[i] = mmbs::bin_key(ref[g], mmb::reg2bin(pos[g], end[g]));
    M[i] = std::max(i ? M[i - 1] : 0, mmbs::end_key(ref[g], end[g]));
    ++ref_start[(size_t)ref[g] + 1];
  }
  for (int32_t r = 0; r < n_ref; ++r) ref_start[r + 1] += ref_start[r];
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return bkey[a] < bkey[b]; });
  std::vector<uint64_t> skey((size_t)n);
  for (int64_t j = 0; j < n; ++j) skey[j] = bkey[ord[j]];
  for (int64_t j = 0; j < n; ++j) {
    if (mmbs::chunk_head(skey.data(), ord.data(), j)) { ckey.push_back(skey[j]); cvs.push_back(vs[ord[j]]); cve.push_back(0); }
    cve.back() = ve[ord[j]];
  }
  for (int32_t r = 0; r < n_ref; ++r) {
    const int64_t a = ref_start[r], b = ref_start[r + 1];
    const int32_t max_end = b > a ? (int32_t)(uint32_t)M[b - 1] : 0;
    if (b > a) { first_vs[r] = vs[a]; last_ve[r] = ve[b - 1]; }
    win_off[r + 1] = win_off[r] + mmbs::n_intervals(max_end);
    for (int64_t w = 0; w < win_off[r + 1] - win_off[r]; ++w) {
      const int64_t i = mmbs::first_above<uint64_t>(M.data(), a, b, mmbs::end_key(r, (int32_t)(w << mmbs::LINEAR_SHIFT)));
      if (i >= b) return 4;
      ioff.push_back(vs[i]);
    }
  }
  const std::vector<uint8_t> bai = mmbs::bai_bytes(mmbs::BaiParts{n_ref, ref_start.data(), first_vs.data(), last_ve.data(), (int64_t)ckey.size(), ckey.data(), cvs.data(), cve.data(),
                                                                 win_off.data(), ioff.data()});
  hex_out(bai.data(), bai.size());
  for (Buf* b : raw) delete b;
  return 0;
}
