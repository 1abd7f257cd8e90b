// Base modifications on the device (mm_seqset_add_mods, mm_mod_events / _merge / _finish; DESIGN.md section 1, "Base modifications"; the definition:
// mm_mods_core.hpp, the text the host test runs).
//   plane    mod_plane_kernel: one wavefront (a 64-thread workgroup) per read that has groups.  Pass 1: a wave scan over each group's skips in tiles of
//            64, 64-bit sums, gives the ordinals (stored saturated to 32 bits).  Pass 2 over the read in tiles of 64 bases: a ballot per letter and a
//            running popcount give each lane its base's ordinal among its letter, a bounded binary search in each group's ordinals tells whether the
//            base is named and gives its ML byte; the lane stores who | prob << 8.  Every trip count is an array length that the host has checked; an
//            ordinal is compared and never used as an index.  A group that names an occurrence beyond the read's count of its base puts
//            (sequence << 8 | group) into the error word with an atomic minimum; the host reads the word and drops the plane.
//   events   mm_events.hpp's pipeline (count, scan, emit, sort, reduce) over one-word keys with ModEvents.  mod_count_kernel: one wavefront per job applies
//            the pileup's rules (mmp::count_job) and counts the calls under the job's = runs — a lane takes a run, all lanes a run of more than 64
//            columns; mod_emit_kernel writes the keys: memory grows with the calls, a base without a call takes no slot.
//   merge    mm_keytable.hip's merge_run over one-word keys (it reads no field of a key).
//   finish   mod_rows_kernel twice: the head of every (contig, position, strand) segment counts its rows from its at most 7 entries and the packed
//            reference's byte, a scan places them, the second launch writes them.
// No kernel here waits for another workgroup; the only atomic is the error words' minimum.
#include "mm_mods.hpp"
#include "mm_events.hpp"
#include "mm_prims.hpp"

namespace mm {

namespace {
constexpr unsigned long long MODS_NO_ERROR = ~0ull;

struct PlaneCalls {                                                // a read's stored calls (null: the set has no plane)
  const uint16_t* p;
  __device__ uint16_t call(int64_t s) const { return p ? p[s] : (uint16_t)0; }
};

// read r of the reads with groups: sequence seq[r] with the groups [goff[r], goff[r + 1])
__global__ void __launch_bounds__(64) mod_plane_kernel(EditSeq Q, const uint64_t* __restrict__ base, const int32_t* __restrict__ len, const int32_t* __restrict__ seq,
                                                       const int64_t* __restrict__ goff, mmd::Groups G, const uint32_t* __restrict__ skips, uint32_t* __restrict__ ord, int64_t r0,
                                                       int64_t n, uint16_t* __restrict__ plane, unsigned long long* __restrict__ err) {
  const int64_t r = r0 + (int64_t)blockIdx.x;
  if (r >= n) return;
  WaveLanes p;
  const int64_t i = seq[r], g0 = goff[r], g1 = goff[r + 1];
  for (int64_t g = g0; g < g1; ++g) mmd::group_ordinals(p, skips + G.soff[g], G.soff[g + 1] - G.soff[g], ord + G.soff[g]);
  __syncthreads();                                                 // (the ordinals are read by other lanes than the ones that stored them)
  const uint64_t b = base[i];
  const int64_t L = len[i];
  const int bad = mmd::plane_read(p, SeqBytes{Q.narrowed(b, b + (uint64_t)L), (int64_t)b}, L, G, g0, g1, plane + b);
  if (threadIdx.x == 0 && bad >= 0) atomicMin(err, (unsigned long long)i << 8 | (unsigned long long)bad);
}

__global__ void __launch_bounds__(64) mod_count_kernel(const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len,
                                                       int64_t n_contigs, AlignedJobs J, const uint8_t* __restrict__ use, const uint16_t* __restrict__ plane, int32_t min_ml, int64_t job0,
                                                       int64_t* __restrict__ counts, unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  WaveLanes p;
  int64_t events = 0;
  int rule = 0;
  if (use[job] && J.dist[job] >= 0) {
    const uint32_t* const ops = J.ops + J.op_off[job];
    const int64_t n_ops = J.op_off[job + 1] - J.op_off[job];
    rule = mmp::count_job(p, J.read[job], n_reads, J.contig[job], n_contigs, J.strand[job], q_len, r_len, J.first[job], ops, n_ops, &events);
    events = 0;
    if (!rule && plane) {                                          // (the rules have passed: every read index of the walk is inside the read)
      const int32_t read = J.read[job];
      events = mmd::walk_job(p, PlaneCalls{plane + q_base[read]}, (int64_t)q_len[read], J.strand[job], (int64_t)J.contig[job], J.first[job], ops, n_ops, min_ml, nullptr);
    }
  }
  if (threadIdx.x == 0) {
    counts[job] = events;
    if (rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
  }
}
// the events of job to keys[off[job], off[job + 1]); a job without events writes nothing
__global__ void __launch_bounds__(64) mod_emit_kernel(const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, AlignedJobs J, const uint16_t* __restrict__ plane,
                                                      int32_t min_ml, int64_t job0, const int64_t* __restrict__ off, uint64_t* __restrict__ keys) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n || off[job + 1] == off[job]) return;
  WaveLanes p;
  const int32_t read = J.read[job];
  mmd::walk_job(p, PlaneCalls{plane + q_base[read]}, (int64_t)q_len[read], J.strand[job], (int64_t)J.contig[job], J.first[job], J.ops + J.op_off[job],
                J.op_off[job + 1] - J.op_off[job], min_ml, keys + off[job]);
}

// rows == nullptr: n_rows[i] = the rows of the segment that entry i starts (0 for an entry inside a segment), n_rows[n] = 0 for the scan's total;
// else the rows to rows[pos[i] ...]
__global__ void __launch_bounds__(256) mod_rows_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, int64_t n, EditSeq R, const uint64_t* __restrict__ r_base,
                                                       mmd::CodeBases cb, int64_t min_coverage, int32_t* __restrict__ n_rows, const int64_t* __restrict__ pos, mmd::Row* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int k = 0;
  if (i < n && (i == 0 || mmd::key_site(keys[i]) != mmd::key_site(keys[i - 1]))) {
    const uint8_t b = R.byte((int64_t)r_base[mmd::key_contig(keys[i])] + mmd::key_pos(keys[i]));
    k = mmd::segment_rows(keys, counts, i, n, b, cb, min_coverage, rows ? rows + pos[i] : nullptr);
  }
  if (!rows) n_rows[i] = k;
}
}  // namespace

void seqset_add_mods(mm_seqset* s, int32_t n_groups, const uint8_t* base, const int8_t* code, const uint8_t* mode, const int64_t* off, const uint32_t* skips, const uint8_t* ml) {
  const std::string w = "mm_seqset_add_mods: ";
  auto& M = s->staged_mods;
  MM_REQUIRE(!s->frozen, MM_ERR_ARG, w + "the sequence set is already uploaded");
  MM_REQUIRE(!s->staged.empty(), MM_ERR_ARG, w + "the set has no sequence yet");
  MM_REQUIRE(M.seq.empty() || (size_t)M.seq.back() + 1 != s->staged.size(), MM_ERR_ARG, w + "the sequence added last has its modifications already");
  MM_REQUIRE(n_groups >= 0 && n_groups <= mmd::MAX_GROUPS, MM_ERR_ARG, w + "n_groups is not in [0, 255]");
  MM_REQUIRE(n_groups == 0 || (base && code && mode && off), MM_ERR_ARG, w + "a null array");
  int64_t k0 = 0, k1 = 0;
  if (n_groups) {
    offsets_check(off, n_groups, "mm_seqset_add_mods", "off");
    k0 = off[0]; k1 = off[n_groups];
    MM_REQUIRE(k1 == k0 || (skips && ml), MM_ERR_ARG, w + "a null array");
    MM_REQUIRE((int64_t)M.skips.size() + (k1 - k0) < ((int64_t)1 << 31), MM_ERR_LIMIT, w + "2^31 skips or more in one set");
  }
  for (int32_t g = 0; g < n_groups; ++g) {
    MM_REQUIRE(base[g] == 'A' || base[g] == 'C' || base[g] == 'G' || base[g] == 'T', MM_ERR_ARG, w + "group " + std::to_string(g) + ": the base is not one of A C G T");
    MM_REQUIRE(code[g] >= -1 && code[g] < mmd::MAX_CODES, MM_ERR_ARG, w + "group " + std::to_string(g) + ": the code is not in [-1, 3]");
    MM_REQUIRE(mode[g] == mmd::MODE_ABSENT || mode[g] == mmd::MODE_DOT || mode[g] == mmd::MODE_ASK, MM_ERR_ARG, w + "group " + std::to_string(g) + ": the mode is not 0, '.' or '?'");
  }
  M.seq.push_back((int32_t)(s->staged.size() - 1));
  for (int32_t g = 0; g < n_groups; ++g) {
    M.base.push_back((uint8_t)mmp::base_code(base[g])); M.code.push_back(code[g]); M.mode.push_back(mode[g]);
    M.soff.push_back(M.soff.back() + (off[g + 1] - off[g]));
  }
  if (k1 > k0) { M.skips.insert(M.skips.end(), skips + k0, skips + k1); M.ml.insert(M.ml.end(), ml + k0, ml + k1); }
  M.goff.push_back((int64_t)M.base.size());
}

void seqset_upload_mods(mm_seqset* s) {
  auto& M = s->staged_mods;
  if (M.seq.empty()) return;                                       // nothing is allocated and nothing launched for a set without modifications
  hipStream_t st = s->ctx->stream;
  StageClock<1> clk(getenv("MM_MODS_TIMING") != nullptr, st);
  const size_t n = s->len.size(), nb = (size_t)s->base[n], R = M.seq.size(), G = M.base.size(), K = M.skips.size();
  clk.start();
  s->has_mods = true;
  s->mods.alloc(nb);
  s->mods.zero(st);
  unsigned long long e = MODS_NO_ERROR;
  if (nb && G) {
    DBuf<int32_t> d_seq(R); DBuf<int64_t> d_goff(R + 1), d_soff(G + 1); DBuf<uint8_t> d_base(G), d_mode(G), d_ml(std::max<size_t>(K, 1)); DBuf<int8_t> d_code(G);
    DBuf<uint32_t> d_skips(std::max<size_t>(K, 1)), d_ord(std::max<size_t>(K, 1)); DBuf<unsigned long long> d_err(1);
    d_seq.upload(M.seq.data(), R, st); d_goff.upload(M.goff.data(), R + 1, st); d_soff.upload(M.soff.data(), G + 1, st);
    d_base.upload(M.base.data(), G, st); d_mode.upload(M.mode.data(), G, st); d_code.upload(M.code.data(), G, st);
    d_ml.upload(M.ml.data(), K, st); d_skips.upload(M.skips.data(), K, st);
    MM_HIP(hipMemsetAsync(d_err.p, 0xFF, sizeof(unsigned long long), st));
    const mmd::Groups Gv{d_base.p, d_code.p, d_mode.p, d_soff.p, d_ord.p, d_ml.p};
    for_job_grids(0, (int64_t)R, [&](int64_t a, dim3 grid) {
      mod_plane_kernel<<<grid, dim3(64), 0, st>>>(edit_seq(s), s->d_base.p, s->d_len.p, d_seq.p, d_goff.p, Gv, d_skips.p, d_ord.p, a, (int64_t)R, s->mods.p, d_err.p);
    });
    e = d_err.to_host(st)[0];
  }
  MM_HIP(mm::stream_sync(st));
  clk.stop(0);
  if (clk.on)
    fprintf(stderr, "MM_MODS_TIMING plane: %.3f ms; %zu sequences with groups, %zu groups, %zu calls, %zu B staged, %zu B plane\n", clk.ms[0], R, G, K,
            R * 12 + G * 11 + K * 5, nb * 2);
  if (e != MODS_NO_ERROR) {
    const size_t i = (size_t)(e >> 8);
    size_t r = (size_t)(std::lower_bound(M.seq.begin(), M.seq.end(), (int32_t)i) - M.seq.begin());
    const size_t g = (size_t)M.goff[r] + (size_t)(e & 255);
    s->has_mods = false; s->mods.release();
    throw Error(MM_ERR_DATA, "mm_seqset_upload: sequence " + std::to_string(i) + ": modification group " + std::to_string((unsigned)(e & 255)) + " names more " +
                                 std::string(1, (char)ascii_of_code(M.base[g])) + " bases than the sequence has");
  }
  M = mm_seqset::StagedMods{};
}

void seqset_fetch_mods(mm_seqset* s, int64_t i, uint8_t* who, uint8_t* prob, int64_t cap) {
  MM_REQUIRE(s->frozen, MM_ERR_STATE, "sequence set not uploaded");
  MM_REQUIRE(i >= 0 && i < s->count(), MM_ERR_ARG, "sequence index out of range");
  const int64_t L = s->len[(size_t)i];
  MM_REQUIRE(cap >= L, MM_ERR_ARG, "output buffer too small");
  if (!L) return;
  std::vector<uint16_t> v((size_t)L, 0);
  if (s->has_mods) {
    hipStream_t st = s->ctx->stream;
    s->mods.download(v.data(), (size_t)L, st, (size_t)s->base[(size_t)i]);
    MM_HIP(mm::stream_sync(st));
  }
  for (int64_t j = 0; j < L; ++j) { who[j] = (uint8_t)(v[(size_t)j] & 255u); prob[j] = (uint8_t)(v[(size_t)j] >> 8); }
}

namespace {
struct ModEvents {                                               // what mm_events.hpp's pipeline asks of a format
  static constexpr const char* who = "mm_mod_events";
  static constexpr const char* timing = "MM_MODS_TIMING";
  static constexpr int32_t param_max = 255;
  static constexpr const char* param_text = "mm_mod_events: min_ml is not in [0, 255]";
  static constexpr int64_t max_contigs = mmd::MAX_CONTIGS;
  static constexpr const char* contigs_text = "mm_mod_events: more than 2^28 contigs";
  static constexpr int key_shift = mmd::CONTIG_SHIFT;
  static constexpr bool two_words = false;
  static constexpr const char* second = nullptr;
  static constexpr uint64_t sentinel = 0;                          // (none: a base without a call takes no slot)
  static bool cuts_sentinel(int32_t) { return false; }
  static int32_t value(const mm_seqset*, int32_t min_ml) { return min_ml; }
  static const char* rule_text(int rule) { return mmp::rule_text(rule); }
  static void count(const EventsLaunch& L, int64_t a, dim3 grid) {
    mod_count_kernel<<<grid, dim3(64), 0, L.st>>>(L.reads->d_base.p, L.reads->d_len.p, L.reads->count(), L.ref->d_len.p, L.ref->count(), L.J, L.use, L.reads->mods_ptr(), L.value, a, L.counts,
                                                  L.err);
  }
  static void emit(const EventsLaunch& L, int64_t a, dim3 grid) {
    mod_emit_kernel<<<grid, dim3(64), 0, L.st>>>(L.reads->d_base.p, L.reads->d_len.p, L.J, L.reads->mods_ptr(), L.value, a, L.off, L.w0);
  }
};
}  // namespace
void mod_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in, const uint8_t* use, int32_t min_ml, KeyTable* out) {
  key_events_run<ModEvents>(ctx, reads, ref, in, use, min_ml, out);
}

mmd::CodeBases mod_table_checks(const std::string& w, mm_ctx* ctx, const mm_seqset* ref, int64_t n, const uint64_t* keys, int32_t n_codes, const uint8_t* code_base,
                                int64_t min_coverage) {
  MM_REQUIRE(ref->frozen, MM_ERR_STATE, w + "the reference is not uploaded");
  MM_REQUIRE(ref->ctx->device == ctx->device, MM_ERR_ARG, w + "the reference lives on another device");
  MM_REQUIRE(ref->count() <= mmd::MAX_CONTIGS, MM_ERR_ARG, w + "more than 2^28 contigs");
  MM_REQUIRE(n_codes >= 1 && n_codes <= mmd::MAX_CODES && code_base, MM_ERR_ARG, w + "n_codes is not in [1, 4]");
  MM_REQUIRE(min_coverage >= 1, MM_ERR_ARG, w + "min_coverage is below 1");
  mmd::CodeBases cb{};
  cb.n = n_codes;
  for (int32_t c = 0; c < n_codes; ++c) {
    MM_REQUIRE(code_base[c] == 'A' || code_base[c] == 'C' || code_base[c] == 'G' || code_base[c] == 'T', MM_ERR_ARG, w + "code " + std::to_string(c) + ": the base is not one of A C G T");
    cb.b[c] = code_base[c];
  }
  for (int64_t i = 0; i < n; ++i) {                                // before anything is launched: every later index is inside its array
    const uint64_t key = keys[i];
    MM_REQUIRE(i == 0 || keys[i - 1] < key, MM_ERR_ARG, w + "the keys are not ascending and unique (entry " + std::to_string(i) + "): pass a merged table");
    MM_REQUIRE(mmd::key_contig(key) < ref->count() && mmd::key_pos(key) < ref->len[(size_t)mmd::key_contig(key)] && mmd::key_class(key) < mmd::CLASS_CODE0 + (uint32_t)n_codes, MM_ERR_ARG,
               w + "entry " + std::to_string(i) + " names no position of the reference, or no class of the asked codes");
  }
  return cb;
}

void mod_finish_run(mm_ctx* ctx, const mm_seqset* ref, int64_t n, const uint64_t* keys, const uint32_t* counts, int32_t n_codes, const uint8_t* code_base, int64_t min_coverage,
                    ModResult* out) {
  const mmd::CodeBases cb = mod_table_checks("mm_mod_finish: ", ctx, ref, n, keys, n_codes, code_base, min_coverage);
  out->site.clear(); out->n_mod.clear(); out->n_canonical.clear(); out->n_other.clear(); out->n_fail.clear();
  if (n == 0) return;
  hipStream_t st = ctx->stream;
  StageClock<1> clk(getenv("MM_MODS_TIMING") != nullptr, st);
  clk.start();
  const size_t k = (size_t)n;
  DBuf<uint64_t> d_keys(k); DBuf<uint32_t> d_counts(k); DBuf<int32_t> d_nrows(k + 1); DBuf<int64_t> d_pos(k + 1); DBuf<uint8_t> tmp;
  d_keys.upload(keys, k, st); d_counts.upload(counts, k, st);
  mod_rows_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(d_keys.p, d_counts.p, n, edit_seq(ref), ref->d_base.p, cb, min_coverage, d_nrows.p, nullptr, nullptr); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_nrows.p, d_pos.p, k + 1, st);
  int64_t total = 0;
  d_pos.download(&total, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  if (total > 0) {
    DBuf<mmd::Row> d_rows((size_t)total);
    mod_rows_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(d_keys.p, d_counts.p, n, edit_seq(ref), ref->d_base.p, cb, min_coverage, d_nrows.p, d_pos.p, d_rows.p); MM_KERNEL_CHECK();
    const std::vector<mmd::Row> rows = d_rows.to_host(st);
    for (const mmd::Row& r : rows) {
      out->site.push_back(r.site); out->n_mod.push_back(r.n_mod); out->n_canonical.push_back(r.n_canonical); out->n_other.push_back(r.n_other);
      out->n_fail.push_back(r.n_fail);
    }
  }
  clk.stop(0);
  if (clk.on) fprintf(stderr, "MM_MODS_TIMING finish: %.3f ms; %lld entries, %zu rows\n", clk.ms[0], (long long)n, out->site.size());
}

}  // namespace mm
