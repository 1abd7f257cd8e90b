// extern "C" surface of libmetamaps_hip.so (include/metamaps_hip.h).  Converts internal exceptions into
// status codes + mm_last_error(); owns handle lifetimes.  No CPU fallback anywhere: without a gfx950
// device mm_ctx_create fails and nothing else can be called.
#include "mm_env.hpp"
#include "mm_map.hpp"
#include "mm_em.hpp"
#include "mm_stats.hpp"
#include "mm_synth.hpp"
#include "mm_hpc.hpp"
#include "mm_lca.hpp"
#include "mm_gene.hpp"
#include "mm_ident.hpp"
#include "mm_edit.hpp"
#include "mm_bam.hpp"
#include "mm_bam_sort.hpp"
#include "mm_reads_out.hpp"
#include "mm_pileup.hpp"
#include "mm_vcf.hpp"
#include "mm_mods.hpp"
#include "mm_motif.hpp"
#include "mm_cons.hpp"
#include "mm_cons_core.hpp"
#include "mm_depth.hpp"
#include "mm_depth_core.hpp"
#include "mm_errprof.hpp"
#include "mm_errprof_core.hpp"
#include "mm_seq.hpp"
#include "mm_codec.hpp"
#include <chrono>
#include <new>

namespace {
// a context is bound to the calling thread for the duration of a call: its device (hipSetDevice is per thread), its
// stream and its allocator.  Several contexts — one per GPU, or several on one GPU — may be driven from different threads.
// (No device is selected while the context has no stream yet: mm_ctx_create's own lambda does that.)  checked: a failing hipSetDevice throws.
void bind(mm_ctx* ctx, bool checked = false) {
  mm::current_stream() = ctx->stream; mm::current_alloc() = &ctx->alloc;
  if (ctx->device < 0 || !ctx->stream) return;
  if (checked) MM_HIP(hipSetDevice(ctx->device)); else (void)hipSetDevice(ctx->device);
}
template <typename F>
int guarded(mm_ctx* ctx, F&& f) {
  try { if (ctx) bind(ctx, true); f(); return MM_OK; }
  catch (const mm::Error& e) { if (ctx) ctx->err = e.what(); return e.status; }
  catch (const std::bad_alloc&) { if (ctx) ctx->err = "host allocation failed"; return MM_ERR_NOMEM; }
  catch (const std::exception& e) { if (ctx) ctx->err = e.what(); return MM_ERR_DEVICE; }
}
// The entry points that hand back a new object: *out is NULL unless they return MM_OK — when the arguments are refused ...
template <typename H> int refused(H** out) { if (out) *out = nullptr; return MM_ERR_ARG; }
template <typename H> auto set_ctx(H& h, mm_ctx* ctx, int) -> decltype((void)(h.ctx = ctx)) { h.ctx = ctx; }
template <typename H> void set_ctx(H&, mm_ctx*, long) {}            // (handles of host memory alone carry no context)
// ... and when making the object fails: fill(object) makes it on the context's device, and *out stays NULL unless fill returns.
template <typename H, typename F>
int created(mm_ctx* ctx, H** out, F&& fill) {
  *out = nullptr;
  return guarded(ctx, [&] {
    std::unique_ptr<H> h(new H());
    set_ctx(*h, ctx, 0);
    fill(*h);
    *out = h.release();
  });
}
// ... and one whose object the callee makes, or declines to make, itself (mm_gzip, whose struct is its unit's own; mm_mapping_gather off the owner)
template <typename H, typename F>
int adopted(mm_ctx* ctx, H** out, F&& make) {
  *out = nullptr;
  return guarded(ctx, [&] { *out = make(); });
}
// what the entry points over aligned jobs, over key tables and over their finishes ask of their counts and arrays (who: the entry point's name)
void require_jobs(const char* who, int64_t n_jobs, bool arrays) {
  MM_REQUIRE(n_jobs >= 0 && n_jobs < ((int64_t)1 << 31), n_jobs < 0 ? MM_ERR_ARG : MM_ERR_LIMIT, std::string(who) + ": a negative number of jobs, or 2^31 or more");
  MM_REQUIRE(n_jobs == 0 || arrays, MM_ERR_ARG, std::string(who) + ": a null array");
}
void require_records(const char* who, int64_t n_rec, bool arrays) {
  MM_REQUIRE(n_rec < ((int64_t)1 << 31), MM_ERR_LIMIT, std::string(who) + ": 2^31 records or more");
  MM_REQUIRE(n_rec == 0 || arrays, MM_ERR_ARG, std::string(who) + ": a null array");
}
void require_rows(const char* who, const char* rows, int64_t n, bool arrays) {
  MM_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), n < 0 ? MM_ERR_ARG : MM_ERR_LIMIT, std::string(who) + ": a negative number of " + rows + ", or 2^32 or more");
  MM_REQUIRE(n == 0 || arrays, MM_ERR_ARG, std::string(who) + ": a null array");
}
void require_finish(const char* who, int64_t n, int64_t n_iv, bool rows, bool intervals) {
  MM_REQUIRE(n >= 0 && n < ((int64_t)1 << 32) && n_iv >= 0 && n_iv < ((int64_t)1 << 32), n < 0 || n_iv < 0 ? MM_ERR_ARG : MM_ERR_LIMIT,
             std::string(who) + ": a negative number of entries or intervals, or 2^32 or more");
  MM_REQUIRE((n == 0 || rows) && (n_iv == 0 || intervals), MM_ERR_ARG, std::string(who) + ": a null array");
}
// The handles of the three key tables (host memory only, as mm_alignment) and the entry points they share; mm_pileup, mm_mod and mm_vcf below are this and
// nothing else.  One-word keys: t.w1 stays empty, and w1 is null in every call.
template <bool TwoWords> struct key_table { static constexpr bool two_words = TwoWords; mm::KeyTable t; };
using EventsRun = void (*)(mm_ctx*, const mm_seqset*, const mm_seqset*, const mm::AlignedJobsIn&, const uint8_t*, int32_t, mm::KeyTable*);
template <typename H>
int table_events(const char* who, EventsRun run, mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const mm::AlignedJobsIn& in, const uint8_t* use, int32_t param, H** out) {
  if (!ctx || !reads || !reference || !out) return refused(out);
  return created(ctx, out, [&](H& h) {
    require_jobs(who, in.n_jobs, in.read && in.strand && in.contig && in.dist && in.first && in.op_off && use);
    run(ctx, reads, reference, in, use, param, &h.t);
  });
}
template <typename H>
int table_merge(const char* who, const char* rows, const char* timing_env, mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, H** out) {
  if (!ctx || !out) return refused(out);
  return created(ctx, out, [&](H& h) {
    require_rows(who, rows, n, w0 && counts && (w1 || !H::two_words));
    mm::merge_run(ctx, n, w0, w1, counts, who, timing_env, &h.t);
  });
}
template <typename H> int table_sizes(const H* h, int64_t* n_rows) {
  if (!h || !n_rows) return MM_ERR_ARG;
  *n_rows = (int64_t)h->t.w0.size();
  return MM_OK;
}
template <typename H> int table_fetch(const H* h, uint64_t* w0, uint64_t* w1, uint32_t* counts) {
  if (!h) return MM_ERR_ARG;
  const mm::KeyTable& t = h->t;
  const size_t k = t.w0.size();
  if (k && (!w0 || !counts || (!t.w1.empty() && !w1))) return MM_ERR_ARG;
  if (k) { memcpy(w0, t.w0.data(), k * 8); memcpy(counts, t.counts.data(), k * 4); }
  if (k && !t.w1.empty()) memcpy(w1, t.w1.data(), k * 8);
  return MM_OK;
}
}  // namespace

extern "C" {

int mm_abi_version(void) { return MM_ABI_VERSION; }

namespace {
// MM_CTX_TRACE=1: what the process' first HIP calls cost (right behind a process that gave back a device-filling index they wait for the driver)
struct CtxTrace {
  const bool on = getenv("MM_CTX_TRACE") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "MM_CTX_TRACE %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};
}  // namespace

int mm_device_count(void) {
  int n = 0;
  CtxTrace tr;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  tr.lap("hipGetDeviceCount");
  return n;
}
int mm_ctx_create(int device_id, mm_ctx** out) {
  if (!out) return MM_ERR_ARG;
  *out = nullptr;
  if (mm::env_strict()) {                                          // MM_STRICT_ENV=1: a MM_* variable the table (mm_env.hpp) does not know is an error, not a silent default
    const std::string bad = mm::env_unknown();
    if (!bad.empty()) { fprintf(stderr, "mm_ctx_create: unknown MM_* environment switch(es): %s (MM_STRICT_ENV is set; the table is metamaps_amd/csrc/mm_env.hpp / INTEGRATION.md)\n", bad.c_str()); return MM_ERR_ARG; }
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MM_ERR_DEVICE;   // no GPU: fail loudly, never fall back
  if (device_id < 0 || device_id >= n) return MM_ERR_ARG;
  mm_ctx* c = new (std::nothrow) mm_ctx;
  if (!c) return MM_ERR_NOMEM;
  c->device = device_id;
  int st = guarded(c, [&] {
    CtxTrace tr;
    MM_HIP(hipSetDevice(device_id));
    tr.lap("hipSetDevice");
    hipDeviceProp_t p;
    MM_HIP(hipGetDeviceProperties(&p, device_id));
    tr.lap("hipGetDeviceProperties");
    MM_REQUIRE(std::string(p.gcnArchName).rfind("gfx950", 0) == 0, MM_ERR_DEVICE,
               std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only");
    c->cus = p.multiProcessorCount;
    MM_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    mm::stream_event_register(c->stream);
    tr.lap("hipStreamCreateWithFlags");
    if (tr.on) { void* q = nullptr; if (hipMalloc(&q, 1 << 20) == hipSuccess) { tr.lap("first hipMalloc (1 MiB)"); (void)hipFree(q); } }
    c->alloc.stream = c->stream;
    mm::alloc_register(&c->alloc, c->device);
  });
  if (st != MM_OK) { delete c; return st; }
  *out = c;
  return MM_OK;
}
void mm_ctx_destroy(mm_ctx* ctx) {
  if (!ctx) return;
  mm::alloc_unregister(&ctx->alloc);                               // first: from here on no other context's thread trims this cache, waits for this stream or finds its event (reclaim, mm_alloc.hpp)
  (void)hipSetDevice(ctx->device);
  (void)mm::stream_sync(ctx->stream);
  ctx->alloc.trim();
  mm::big_pool_trim(ctx->device);                                  // (recycled index-scale blocks go back to the driver with any context of the device)
  mm::comm_destroy(ctx);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pinned_up) (void)hipHostFree(ctx->pinned_up);
  ctx->l2_lists.release(); ctx->l2_masks.release();
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->aux_stream) { mm::stream_event_unregister(ctx->aux_stream); (void)hipStreamDestroy(ctx->aux_stream); }
  if (ctx->stream) { mm::stream_event_unregister(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
  delete ctx;
}
const char* mm_last_error(const mm_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int mm_ctx_device_info(mm_ctx* ctx, char* name, size_t name_cap, int* cus, uint64_t* hbm_total, uint64_t* hbm_free) {
  if (!ctx) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    hipDeviceProp_t p;
    MM_HIP(hipGetDeviceProperties(&p, ctx->device));
    if (name && name_cap) { snprintf(name, name_cap, "%s (%s)", p.name, p.gcnArchName); }
    if (cus) *cus = p.multiProcessorCount;
    size_t f = 0, t = 0;
    MM_HIP(mm::dev_mem_info(&f, &t));                             // (capped by the test hook MM_DEVICE_BYTES_CAP, mm_alloc.hpp)
    if (hbm_total) *hbm_total = t;
    if (hbm_free) *hbm_free = f;
  });
}
int mm_ctx_synchronize(mm_ctx* ctx) {
  if (!ctx) return MM_ERR_ARG;
  return guarded(ctx, [&] { MM_HIP(mm::stream_sync(ctx->stream)); });
}
int mm_ctx_release_cached(mm_ctx* ctx) {
  if (!ctx) return MM_ERR_ARG;
  return guarded(ctx, [&] { ctx->alloc.trim(); mm::big_pool_trim(ctx->device); });
}
void* mm_ctx_stream(mm_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

// ---- sequences ----------------------------------------------------------------------------------------
int mm_seqset_create(mm_ctx* ctx, mm_seqset** out) {
  if (!ctx || !out) return refused(out);
  return created(ctx, out, [](mm_seqset&) {});
}
void mm_seqset_destroy(mm_seqset* s) { if (s) { bind(s->ctx); delete s; } }
int mm_seqset_add(mm_seqset* s, const char* ascii, int64_t len) {
  if (!s || (!ascii && len > 0) || len < 0) return MM_ERR_ARG;
  return guarded(s->ctx, [&] {
    MM_REQUIRE(!s->frozen, MM_ERR_STATE, "sequence set already uploaded");
    MM_REQUIRE(s->staged_kind != 2, MM_ERR_STATE, "this sequence set holds 4-bit codes (mm_seqset_add_nt16): ASCII cannot join it");
    s->staged_kind = 1;
    s->owned.emplace_back(ascii ? ascii : "", (size_t)len);
    s->staged.emplace_back(s->owned.back().data(), (size_t)len);
  });
}
int mm_seqset_add_view(mm_seqset* s, const char* ascii, int64_t len) {
  if (!s || (!ascii && len > 0) || len < 0) return MM_ERR_ARG;
  return guarded(s->ctx, [&] {
    MM_REQUIRE(!s->frozen, MM_ERR_STATE, "sequence set already uploaded");
    MM_REQUIRE(s->staged_kind != 2, MM_ERR_STATE, "this sequence set holds 4-bit codes (mm_seqset_add_nt16): ASCII cannot join it");
    s->staged_kind = 1;
    s->staged.emplace_back(ascii, (size_t)len);
  });
}
int mm_seqset_add_nt16(mm_seqset* s, const uint8_t* nt16, int64_t n_bases, int reverse) {
  if (!s || (!nt16 && n_bases > 0) || n_bases < 0) return MM_ERR_ARG;
  return guarded(s->ctx, [&] {
    MM_REQUIRE(!s->frozen, MM_ERR_STATE, "sequence set already uploaded");
    MM_REQUIRE(s->staged_kind != 1, MM_ERR_STATE, "this sequence set holds ASCII sequences: 4-bit codes (mm_seqset_add_nt16) cannot join it");
    s->staged_kind = 2;
    s->staged.emplace_back((const char*)nt16, (size_t)n_bases);
    s->staged_rev.push_back(reverse ? 1 : 0);
  });
}
int mm_seqset_add_qual(mm_seqset* s, const uint8_t* qual, int64_t len, int offset) {
  if (!s || (!qual && len > 0) || len < 0) return MM_ERR_ARG;
  return guarded(s->ctx, [&] {
    MM_REQUIRE(!s->frozen, MM_ERR_ARG, "mm_seqset_add_qual: the sequence set is already uploaded");
    MM_REQUIRE(!s->staged.empty(), MM_ERR_ARG, "mm_seqset_add_qual: the set has no sequence yet");
    MM_REQUIRE(offset == 0 || offset == 33, MM_ERR_ARG, "mm_seqset_add_qual: offset is not 0 or 33");
    MM_REQUIRE((size_t)len == s->staged.back().second, MM_ERR_ARG, "mm_seqset_add_qual: len is not the length of the sequence added last");
    s->staged_qual.resize(s->staged.size());
    MM_REQUIRE(!s->staged_qual.back().set, MM_ERR_ARG, "mm_seqset_add_qual: the sequence added last has its qualities already");
    s->staged_qual.back() = mm_seqset::StagedQual{qual, offset, true};
  });
}
int mm_seqset_has_qual(const mm_seqset* s) {
  if (!s) return 0;
  if (s->frozen) return s->has_qual ? 1 : 0;
  for (const auto& q : s->staged_qual) if (q.set) return 1;
  return 0;
}
int mm_seqset_fetch_qual(mm_seqset* s, int64_t i, uint8_t* out, int64_t cap) {
  if (!s || (!out && cap > 0)) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { mm::seqset_fetch_qual(s, i, out, cap); });
}
int mm_seqset_add_mods(mm_seqset* s, int32_t n_groups, const uint8_t* base, const int8_t* code, const uint8_t* mode, const int64_t* off, const uint32_t* skips, const uint8_t* ml) {
  if (!s) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { mm::seqset_add_mods(s, n_groups, base, code, mode, off, skips, ml); });
}
int mm_seqset_has_mods(const mm_seqset* s) {
  if (!s) return 0;
  return s->frozen ? (s->has_mods ? 1 : 0) : (s->staged_mods.seq.empty() ? 0 : 1);
}
int mm_seqset_fetch_mods(mm_seqset* s, int64_t i, uint8_t* who_out, uint8_t* prob_out, int64_t cap) {
  if (!s || ((!who_out || !prob_out) && cap > 0)) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { mm::seqset_fetch_mods(s, i, who_out, prob_out, cap); });
}
int mm_bgzf_inflate(mm_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, const int64_t* comp_off, const int32_t* comp_len, int32_t n,
                    uint8_t* out, int64_t out_cap, const int64_t* out_off, int32_t* status) {
  if (!ctx || n < 0 || comp_bytes < 0 || out_cap < 0 || (n > 0 && (!comp || !comp_off || !comp_len || !out_off)) || (!out && out_cap > 0)) return MM_ERR_ARG;
  int64_t bad = 0;
  const int rc = guarded(ctx, [&] { bad = mm::bgzf_inflate(ctx, comp, comp_bytes, comp_off, comp_len, n, out, out_cap, out_off, status); });
  if (rc != MM_OK) return rc;
  if (bad) { ctx->err = "mm_bgzf_inflate: " + std::to_string(bad) + " corrupt BGZF block(s)"; return MM_ERR_DATA; }
  return MM_OK;
}
int64_t mm_bgzf_deflate_bound(int64_t in_bytes) { return in_bytes < 0 ? 0 : mm::bgzf_deflate_bound(in_bytes); }
int mm_bgzf_deflate(mm_ctx* ctx, const uint8_t* in, int64_t in_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int32_t* n_blocks) {
  if (!ctx || !out_bytes || !n_blocks || in_bytes < 0 || (in_bytes > 0 && (!in || !out))) return MM_ERR_ARG;
  return guarded(ctx, [&] { mm::bgzf_deflate(ctx, in, in_bytes, out, out_cap, out_bytes, n_blocks); });
}
int mm_gzip_open(mm_ctx* ctx, int64_t chunk_bytes, int64_t segment_bytes, mm_gzip** out) {
  if (!ctx || !out || chunk_bytes < 0 || segment_bytes < 0) return refused(out);
  return adopted(ctx, out, [&] { return mm::gzip_open(ctx, chunk_bytes, segment_bytes); });
}
int mm_gzip_feed(mm_gzip* g, const uint8_t* comp, int64_t n, int last, int64_t* avail) {
  if (!g || n < 0 || (n > 0 && !comp)) return MM_ERR_ARG;
  int bad = 0;
  const int rc = guarded(mm::gzip_ctx(g), [&] { bad = mm::gzip_feed(g, comp, n, last != 0, avail); });
  if (rc != MM_OK) return rc;
  return bad ? MM_ERR_DATA : MM_OK;
}
int mm_gzip_read(mm_gzip* g, uint8_t* out, int64_t cap, int64_t* got) {
  if (!g || cap < 0 || (cap > 0 && !out) || !got) return MM_ERR_ARG;
  *got = mm::gzip_read(g, out, cap);
  return MM_OK;
}
int mm_gzip_stats(const mm_gzip* g, int64_t* counts, double* seconds) {
  if (!g) return MM_ERR_ARG;
  mm::gzip_stats(g, counts, seconds);
  return MM_OK;
}
void mm_gzip_close(mm_gzip* g) {
  if (!g) return;
  mm_ctx* ctx = mm::gzip_ctx(g);
  (void)guarded(ctx, [&] { mm::gzip_close(g); });
}
int mm_seqset_upload(mm_seqset* s) {
  if (!s) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { if (s->staged_kind == 2) mm::seqset_upload_nt16(s); else mm::seqset_upload(s); });
}
int mm_seqset_save(mm_seqset* s, const char* path) {
  if (!s || !path) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { mm::seqset_save(s, path); });
}
int mm_seqset_load(mm_ctx* ctx, const char* path, mm_seqset** out) {
  if (!ctx || !path || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& S) { mm::seqset_load(&S, path); });
}
int mm_seqset_slice(mm_ctx* ctx, const mm_seqset* set, int64_t first, int64_t count, mm_seqset** out) {
  if (!ctx || !set || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& S) {
    MM_REQUIRE(set->ctx->device == ctx->device, MM_ERR_ARG, "mm_seqset_slice: the set lives on another device than the context");
    mm::seqset_slice(set, first, count, &S);
  });
}
int mm_seqset_concat(mm_ctx* ctx, const mm_seqset* const* parts, int n_parts, mm_seqset** out) {
  if (!ctx || !parts || n_parts <= 0 || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& S) { mm::seqset_concat(parts, n_parts, &S); });
}
int64_t mm_seqset_count(const mm_seqset* s) { return s ? (s->frozen ? s->count() : (int64_t)s->staged.size()) : 0; }
int64_t mm_seqset_total_bases(const mm_seqset* s) { return s ? s->total_bases : 0; }
int mm_seqset_lengths(const mm_seqset* s, int32_t* len_out) {
  if (!s || !len_out || !s->frozen) return MM_ERR_ARG;
  memcpy(len_out, s->len.data(), s->len.size() * sizeof(int32_t));
  return MM_OK;
}
int mm_seqset_fetch(mm_seqset* s, int64_t i, char* ascii_out, int64_t cap) {
  if (!s || !ascii_out) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { mm::seqset_fetch(s, i, ascii_out, cap); });
}

int mm_seqset_fetch_range(mm_seqset* s, int64_t first, int64_t count, char* ascii_out, int64_t cap) {
  if (!s || (!ascii_out && cap > 0)) return MM_ERR_ARG;
  return guarded(s->ctx, [&] { mm::seqset_fetch_range(s, first, count, ascii_out, cap); });
}

// ---- homopolymer compression (mm_hpc.hip) -------------------------------------------------------------
int mm_seqset_hpc(mm_ctx* ctx, const mm_seqset* raw, mm_seqset** out, mm_hpc_map** map) {
  if (map) *map = nullptr;
  if (!ctx || !raw || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& S) {                  // (two objects: the map is let go only where the set is, behind the last call that can throw)
    std::unique_ptr<mm_hpc_map> M(map ? new mm_hpc_map : nullptr);
    mm::seqset_hpc(ctx, raw, &S, M.get());
    if (map) *map = M.release();
  });
}
int mm_hpc_map_to_raw(mm_hpc_map* map, const int32_t* seq, const int64_t* pos, int64_t n, int64_t* first_out, int64_t* last_out) {
  if (!map || n < 0 || (n > 0 && (!seq || !pos || !first_out || !last_out))) return MM_ERR_ARG;
  return guarded(map->ctx, [&] { mm::hpc_map_to_raw(map, seq, pos, n, first_out, last_out); });
}
int mm_hpc_map_lengths(const mm_hpc_map* map, int32_t* raw_len, int32_t* compressed_len) {
  if (!map) return MM_ERR_ARG;
  if (raw_len) memcpy(raw_len, map->rawlen.data(), map->rawlen.size() * sizeof(int32_t));
  if (compressed_len) memcpy(compressed_len, map->clen.data(), map->clen.size() * sizeof(int32_t));
  return MM_OK;
}
int64_t mm_hpc_map_device_bytes(const mm_hpc_map* map) { return map ? (int64_t)map->device_bytes() : 0; }
int mm_mapping_to_raw(mm_ctx* ctx, mm_mapping* m, const mm_hpc_map* ref_map, int64_t* end_out, int64_t cap) {
  if (!ctx || !m || !ref_map || cap < 0 || (!end_out && cap > 0)) return MM_ERR_ARG;
  return guarded(ctx, [&] { mm::mapping_to_raw(ctx, m, ref_map, end_out, cap); });
}
void mm_hpc_map_destroy(mm_hpc_map* map) { if (map) { bind(map->ctx); delete map; } }

int mm_synth_reference(mm_ctx* ctx, const mm_synth_ref_params* p, mm_seqset** out) {
  if (!ctx || !p || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& s) { mm::synth_reference(ctx, *p, &s); });
}
int mm_synth_community(mm_ctx* ctx, const mm_synth_community_params* p, mm_seqset** out, int32_t* contig_genome) {
  if (!ctx || !p || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& s) { mm::synth_community(ctx, *p, &s, contig_genome); });
}
int mm_synth_community_species(const mm_synth_community_params* p, int32_t* genome_species) {
  if (!p || !genome_species) return MM_ERR_ARG;
  return guarded(nullptr, [&] { mm::synth_community_species(*p, genome_species); });
}
int mm_synth_reads(mm_ctx* ctx, const mm_seqset* reference, const mm_synth_read_params* p, mm_seqset** out, int32_t* truth_genome) {
  if (!ctx || !reference || !p || !out) return refused(out);
  return created(ctx, out, [&](mm_seqset& s) { mm::synth_reads(ctx, reference, *p, &s, truth_genome); });
}

// ---- minimizer tap ------------------------------------------------------------------------------------
int mm_minimizers(mm_ctx* ctx, const mm_seqset* s, int k, int w, int64_t* offsets, uint32_t* hash, int32_t* wpos, int32_t* strand, int64_t cap) {
  if (!ctx || !s) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    mm::MinimizerSet ms;
    mm::run_minimizers(ctx, s, k, w, {}, false, ms);
    if (offsets) for (size_t i = 0; i < ms.h_off.size(); ++i) offsets[i] = (int64_t)ms.h_off[i];
    if (hash || wpos || strand) {
      MM_REQUIRE(cap >= ms.total, MM_ERR_ARG, "output capacity too small");
      auto h = ms.rec.to_host(ctx->stream, (size_t)ms.total);
      for (int64_t i = 0; i < ms.total; ++i) {
        if (hash) hash[i] = h[(size_t)i].hash;
        if (wpos) wpos[i] = mm::pw_wpos(h[(size_t)i].pw);
        if (strand) strand[i] = mm::pw_strand(h[(size_t)i].pw);
      }
    }
  });
}

// ---- index --------------------------------------------------------------------------------------------
int mm_index_build(mm_ctx* ctx, const mm_seqset* contigs, int k, int w, mm_index** out) {
  if (!ctx || !contigs || !out) return refused(out);
  return created(ctx, out, [&](mm_index& I) { mm::index_build(ctx, contigs, k, w, &I); });
}
int mm_index_plan_chunks(mm_ctx* ctx, const mm_index* whole, uint64_t max_memory_bytes, int32_t* first_contig, int32_t cap, int32_t* n_chunks) {
  if (!ctx || !whole || !n_chunks) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    std::vector<int32_t> fc;
    mm::index_plan_chunks(ctx, whole, max_memory_bytes, fc);
    *n_chunks = (int32_t)fc.size();
    if (first_contig) {
      MM_REQUIRE(cap >= (int32_t)fc.size(), MM_ERR_ARG, "output capacity too small");
      for (size_t i = 0; i < fc.size(); ++i) first_contig[i] = fc[i];
    }
  });
}
int mm_index_save(mm_index* idx, const char* path) {
  if (!idx || !path) return MM_ERR_ARG;
  return guarded(idx->ctx, [&] { mm::index_save(idx, path); });
}
int mm_index_load(mm_ctx* ctx, const char* path, mm_index** out) {
  if (!ctx || !path || !out) return refused(out);
  return created(ctx, out, [&](mm_index& I) { mm::index_load(ctx, path, &I); });
}
void mm_index_destroy(mm_index* idx) { if (idx) { bind(idx->ctx); delete idx; } }
int mm_index_get_info(const mm_index* idx, mm_index_info* out) {
  if (!idx || !out) return MM_ERR_ARG;
  out->n_contigs = idx->n_contigs; out->n_entries = idx->N; out->n_unique_hashes = idx->U; out->n_dup_flagged = idx->n_dup;
  out->hbm_bytes = idx->hbm_bytes();
  return MM_OK;
}
int mm_index_freq_hist(mm_index* idx, int64_t* counts, int64_t* n_hashes, int64_t cap, int64_t* n_out) {
  if (!idx || !n_out) return MM_ERR_ARG;
  *n_out = (int64_t)idx->hist.size();
  if (!counts || !n_hashes) return MM_OK;
  if (cap < *n_out) return MM_ERR_ARG;
  int64_t i = 0;
  for (auto& kv : idx->hist) { counts[i] = kv.first; n_hashes[i] = kv.second; ++i; }
  return MM_OK;
}
int mm_freq_threshold_from_hist(const int64_t* counts, const int64_t* n_hashes, int64_t n, int64_t n_unique_hashes, int prev_threshold) {
  return mm::stats::freq_threshold_from_hist(counts, n_hashes, n, n_unique_hashes, prev_threshold);
}
int mm_index_set_freq_threshold(mm_index* idx, int threshold) {
  if (!idx) return MM_ERR_ARG;
  idx->freq_threshold = threshold;
  return MM_OK;
}
int mm_index_entries(mm_index* idx, uint32_t* hash, int32_t* contig, int32_t* wpos, int32_t* strand, int64_t cap) {
  if (!idx) return MM_ERR_ARG;
  return guarded(idx->ctx, [&] { mm::index_entries(idx, hash, contig, wpos, strand, cap); });
}
int mm_index_dup_neighbours(mm_index* idx, int32_t* prev_dist, int32_t* next_dist, int64_t cap) {
  if (!idx || !prev_dist || !next_dist) return MM_ERR_ARG;
  return guarded(idx->ctx, [&] { mm::index_dup_neighbours(idx, prev_dist, next_dist, cap); });
}

// ---- statistics ---------------------------------------------------------------------------------------
int mm_recommended_window(double p_value, int k, float pi, int min_read_len, uint64_t reference_size) {
  return mm::stats::recommended_window(p_value, k, 4, pi, min_read_len, reference_size);
}
double mm_estimate_pvalue(int s, int k, float pi, int min_read_len, uint64_t reference_size) {
  return mm::stats::estimate_pvalue(s, k, 4, pi, min_read_len, reference_size);
}
int mm_min_hits_relaxed(int s, int k, float pi) { return mm::stats::min_hits_relaxed(s, k, pi); }
void mm_identity(int shared, int s, int k, float* ident, float* ident_upper) {
  if (!ident_upper) {                                            // the estimate alone needs no binomial quantile
    if (ident) *ident = 100 * (1 - mm::stats::j2md(1.0 * shared / s, k));
    return;
  }
  float a, b;
  mm::stats::identity(shared, s, k, &a, &b);
  if (ident) *ident = a;
  *ident_upper = b;
}

// ---- mapping ------------------------------------------------------------------------------------------
int mm_map_batch(mm_ctx* ctx, const mm_index* idx, const mm_seqset* reads, const mm_map_params* p, mm_mapping** out) {
  if (!ctx || !idx || !reads || !p || !out) return refused(out);
  return created(ctx, out, [&](mm_mapping& M) {
    MM_REQUIRE(idx->ctx->device == ctx->device, MM_ERR_ARG, "mm_map_batch: the index lives on another device than the context");
    MM_REQUIRE(reads->ctx->device == ctx->device, MM_ERR_ARG, "mm_map_batch: the reads live on another device than the context");
    mm::map_batch(ctx, idx, reads, *p, &M);
  });
}
int mm_map_batch_reusing(mm_ctx* ctx, const mm_index* idx, const mm_seqset* reads, const mm_map_params* p, const mm_mapping* sketch_of, mm_mapping** out) {
  if (!ctx || !idx || !reads || !p || !sketch_of || !out) return refused(out);
  return created(ctx, out, [&](mm_mapping& M) {
    MM_REQUIRE(idx->ctx->device == ctx->device && reads->ctx->device == ctx->device && sketch_of->ctx->device == ctx->device, MM_ERR_ARG,
               "mm_map_batch_reusing: index, reads and donor mapping must live on the context's device");
    MM_REQUIRE(!sketch_of->released, MM_ERR_STATE, "mm_map_batch_reusing: the donor mapping has released its intermediates");
    MM_REQUIRE(sketch_of->n_reads == reads->count() && sketch_of->read_len == reads->len && sketch_of->params.k == p->k && sketch_of->params.w == p->w &&
               sketch_of->params.min_read_len == p->min_read_len, MM_ERR_ARG, "mm_map_batch_reusing: the donor mapping is of other reads or other parameters");
    M.sketch_donor = sketch_of;
    mm::map_batch(ctx, idx, reads, *p, &M);
    M.sketch_donor = nullptr;
  });
}
int mm_sketch_batch(mm_ctx* ctx, const mm_seqset* reads, const mm_map_params* p, mm_mapping** out) {
  if (!ctx || !reads || !p || !out) return refused(out);
  return created(ctx, out, [&](mm_mapping& M) {
    MM_REQUIRE(reads->ctx->device == ctx->device, MM_ERR_ARG, "mm_sketch_batch: the reads live on another device than the context");
    M.sketch_only = true;
    mm::map_batch(ctx, nullptr, reads, *p, &M);
  });
}
int mm_map_batch_phased(mm_ctx* ctx, const mm_index* idx, const mm_seqset* reads, const mm_map_params* p, void (*at_stage)(void*, int), void* user, mm_mapping** out) {
  if (!ctx || !idx || !reads || !p || !out) return refused(out);
  return created(ctx, out, [&](mm_mapping& M) {
    MM_REQUIRE(idx->ctx->device == ctx->device, MM_ERR_ARG, "mm_map_batch_phased: the index lives on another device than the context");
    MM_REQUIRE(reads->ctx->device == ctx->device, MM_ERR_ARG, "mm_map_batch_phased: the reads live on another device than the context");
    M.at_stage = at_stage; M.at_stage_user = user;
    mm::map_batch(ctx, idx, reads, *p, &M);
  });
}
void mm_mapping_destroy(mm_mapping* m) { if (m) { bind(m->ctx); delete m; } }
int mm_mapping_release_intermediates(mm_mapping* m) {
  if (!m) return MM_ERR_ARG;
  return guarded(m->ctx, [&] { m->release_intermediates(); });
}
int mm_mapping_get_stats(const mm_mapping* m, mm_map_stats* out) {
  if (!m || !out) return MM_ERR_ARG;
  *out = m->stats;
  return MM_OK;
}
int mm_mapping_fetch(mm_mapping* m, int64_t* offsets, mm_map_record* records, int64_t cap) {
  if (!m) return MM_ERR_ARG;
  return guarded(m->ctx, [&] {
    if (offsets) for (size_t i = 0; i < m->h_rec_off.size(); ++i) offsets[i] = (int64_t)m->h_rec_off[i];
    if (records) {
      MM_REQUIRE(cap >= m->n_rec, MM_ERR_ARG, "output capacity too small");
      const size_t bytes = (size_t)m->n_rec * sizeof(mm_map_record);
      if (bytes) {                                               // device -> pinned bounce buffer -> caller memory
        void* pin = m->ctx->pinned_at_least(bytes);
        MM_HIP(hipMemcpyAsync(pin, m->rec.p, bytes, hipMemcpyDeviceToHost, m->ctx->stream));
        MM_HIP(mm::stream_sync(m->ctx->stream));
        memcpy(records, pin, bytes);
      }
    }
  });
}
int mm_mapping_add_qualities(mm_ctx* ctx, mm_mapping* m, const mm_seqset* reads, int k) {
  if (!ctx || !m) return MM_ERR_ARG;
  (void)reads;
  return guarded(ctx, [&] { mm::mapping_add_qualities(ctx, m, k); });
}
// ---- read-wise merge of chunk mappings (mm_merge.hip) --------------------------------------------------
int mm_mapping_concat(mm_ctx* ctx, mm_mapping* const* parts, const int32_t* contig_base, int n_parts, mm_mapping** out) {
  if (!ctx || !parts || n_parts <= 0 || !out) return refused(out);
  return created(ctx, out, [&](mm_mapping& M) { mm::mapping_concat(ctx, parts, contig_base, n_parts, &M); });
}
int mm_mapping_from_parts(mm_ctx* ctx, int64_t n_reads, const int32_t* read_len, const mm_map_params* p, int n_parts,
                          const int64_t* const* offsets, const mm_map_record* const* records, const int32_t* contig_base, mm_mapping** out) {
  if (!ctx || n_reads < 0 || (!read_len && n_reads > 0) || !p || n_parts <= 0 || !offsets || !records || !out) return refused(out);
  for (int i = 0; i < n_parts; ++i) if (!offsets[i] || (!records[i] && offsets[i][n_reads] > 0)) return refused(out);
  return created(ctx, out, [&](mm_mapping& M) { mm::mapping_from_parts(ctx, n_reads, read_len, *p, n_parts, offsets, records, contig_base, &M); });
}
int mm_mapping_gather(mm_ctx* ctx, int owner, int64_t n_reads, const int32_t* read_len, const mm_map_params* p, mm_mapping* const* parts, const int32_t* chunk_id,
                      int n_parts, int n_chunks, const int32_t* chunk_rank, const int32_t* contig_base, mm_mapping** out) {
  if (!ctx || !p || n_reads < 0 || (!read_len && n_reads > 0) || n_parts < 0 || (n_parts > 0 && (!parts || !chunk_id)) || n_chunks <= 0 || !chunk_rank || !out) return refused(out);
  return adopted(ctx, out, [&]() -> mm_mapping* {               // (NULL without an error on every rank but the owner)
    std::unique_ptr<mm_mapping> M(new mm_mapping);
    return mm::mapping_gather(ctx, owner, n_reads, read_len, *p, parts, chunk_id, n_parts, n_chunks, chunk_rank, contig_base, M.get()) ? M.release() : nullptr;
  });
}

int mm_mapping_keep_best(mm_ctx* ctx, mm_mapping* m, int k) {
  if (!ctx || !m) return MM_ERR_ARG;
  return guarded(ctx, [&] { mm::mapping_keep_best(ctx, m, k); });
}

int mm_debug_sketch(mm_mapping* m, int64_t* offsets, uint32_t* hash, int32_t* strand, int64_t cap) {
  if (m && m->released) return MM_ERR_STATE;
  if (!m) return MM_ERR_ARG;
  return guarded(m->ctx, [&] {
    hipStream_t st = m->ctx->stream;
    int64_t tot = 0;
    for (int64_t r = 0; r < m->n_reads; ++r) { if (offsets) offsets[r] = tot; tot += m->h_sk_n[(size_t)r]; }
    if (offsets) offsets[m->n_reads] = tot;
    if (!hash && !strand) return;
    MM_REQUIRE(cap >= tot, MM_ERR_ARG, "output capacity too small");
    auto hh = m->sk_hash.to_host(st); auto hs = m->sk_strand.to_host(st);
    int64_t o = 0;
    for (int64_t r = 0; r < m->n_reads; ++r)
      for (int i = 0; i < m->h_sk_n[(size_t)r]; ++i, ++o) {
        size_t src = (size_t)m->mz.h_off[(size_t)r] + (size_t)i;
        if (hash) hash[o] = hh[src];
        if (strand) strand[o] = (hs[src] & 1) ? 1 : -1;       // (bit 1: duplicate of the other strand not resolved, mm_map.hip K2)
      }
  });
}
int mm_debug_hits(mm_mapping* m, int64_t* offsets, int32_t* contig, int32_t* wpos, int64_t cap) {
  if (m && m->released) return MM_ERR_STATE;
  if (!m) return MM_ERR_ARG;
  return guarded(m->ctx, [&] {
    const int64_t tot = (int64_t)m->h_read_hit_off[(size_t)m->n_reads];
    if (offsets) for (size_t i = 0; i < m->h_read_hit_off.size(); ++i) offsets[i] = (int64_t)m->h_read_hit_off[i];
    if (!contig && !wpos) return;
    MM_REQUIRE(cap >= tot, MM_ERR_ARG, "output capacity too small");
    auto h = m->hits.to_host(m->ctx->stream, (size_t)tot);
    for (int64_t i = 0; i < tot; ++i) {
      if (contig) contig[i] = (int32_t)(h[(size_t)i] >> 32);
      if (wpos) wpos[i] = mm::pw_wpos((uint32_t)h[(size_t)i]);
    }
  });
}
int mm_debug_candidates(mm_mapping* m, int64_t* offsets, int32_t* triples, int64_t cap) {
  if (m && m->released) return MM_ERR_STATE;
  if (!m) return MM_ERR_ARG;
  return guarded(m->ctx, [&] {
    if (offsets) for (size_t i = 0; i < m->h_cand_off.size(); ++i) offsets[i] = (int64_t)m->h_cand_off[i];
    if (!triples) return;
    MM_REQUIRE(cap >= m->n_cand, MM_ERR_ARG, "output capacity too small");
    m->cand.download(triples, (size_t)(3 * m->n_cand), m->ctx->stream);
    MM_HIP(mm::stream_sync(m->ctx->stream));
  });
}
int mm_debug_l2(mm_mapping* m, int64_t* per_cand, int64_t cap) {
  if (m && m->released) return MM_ERR_STATE;
  if (!m || !per_cand) return MM_ERR_ARG;
  return guarded(m->ctx, [&] {
    MM_REQUIRE(cap >= m->n_cand, MM_ERR_ARG, "output capacity too small");
    auto h = m->l2.to_host(m->ctx->stream, (size_t)m->n_cand);
    for (int64_t i = 0; i < m->n_cand; ++i) {
      per_cand[6 * i] = h[(size_t)i].contig; per_cand[6 * i + 1] = h[(size_t)i].mean_pos; per_cand[6 * i + 2] = h[(size_t)i].shared;
      per_cand[6 * i + 3] = h[(size_t)i].opt_beg; per_cand[6 * i + 4] = h[(size_t)i].opt_end; per_cand[6 * i + 5] = h[(size_t)i].accepted;
    }
  });
}
int mm_debug_min_hits(mm_mapping* m, int32_t* min_hits) {
  if (m && m->released) return MM_ERR_STATE;
  if (!m || !min_hits) return MM_ERR_ARG;
  memcpy(min_hits, m->h_min_hits.data(), m->h_min_hits.size() * sizeof(int32_t));
  return MM_OK;
}

int mm_debug_probed_lists(mm_mapping* m, const mm_index* idx, int64_t* hist, int32_t n_bins) {
  if (m && m->released) return MM_ERR_STATE;
  if (!m || !idx || !hist || n_bins < 3) return MM_ERR_ARG;
  return guarded(m->ctx, [&] { mm::probed_list_hist(m->ctx, idx, m, n_bins, hist); });
}

// ---- EM -----------------------------------------------------------------------------------------------
int mm_em_create(mm_ctx* ctx, int64_t n_reads, const int64_t* read_off, const int32_t* taxon, const double* mapq, const double* inv_nloc,
                 int32_t n_taxa, mm_em** out) {
  if (!ctx || !read_off || !out || n_reads < 0 || n_taxa <= 0) return refused(out);
  return created(ctx, out, [&](mm_em& E) { mm::em_create(ctx, n_reads, read_off, taxon, mapq, inv_nloc, n_taxa, &E); });
}
int mm_em_create_from_mapping(mm_ctx* ctx, const mm_mapping* m, const int32_t* contig_taxon, const int32_t* contig_len, int32_t n_contigs,
                              int32_t n_taxa, mm_em** out) {
  if (!ctx || !m || !contig_taxon || !contig_len || !out || n_contigs < 0 || n_taxa <= 0) return refused(out);
  return created(ctx, out, [&](mm_em& E) { mm::em_create_from_mapping(ctx, m, contig_taxon, contig_len, n_contigs, n_taxa, &E); });
}
int mm_em_taxon_counts(mm_em* em, int64_t* counts) {
  if (!em || !counts) return MM_ERR_ARG;
  return guarded(em->ctx, [&] {
    auto ts = em->tstart.to_host(em->ctx->stream, (size_t)em->n_taxa + 1);
    for (int32_t t = 0; t < em->n_taxa; ++t) counts[t] = ts[(size_t)t + 1] - ts[(size_t)t];
  });
}
int mm_em_sizes(const mm_em* em, int64_t* n_reads, int64_t* n_entries, int32_t* n_taxa) {
  if (!em) return MM_ERR_ARG;
  if (n_reads) *n_reads = em->n_reads;
  if (n_entries) *n_entries = em->n_entries;
  if (n_taxa) *n_taxa = em->n_taxa;
  return MM_OK;
}
void mm_em_destroy(mm_em* em) { if (em) { bind(em->ctx); delete em; } }
int mm_em_iterate(mm_em* em, const double* f, double* f_partial, double* ll_partial) {
  if (!em || !f || !f_partial || !ll_partial) return MM_ERR_ARG;
  return guarded(em->ctx, [&] { mm::em_iterate(em, f, f_partial, ll_partial); });
}
int mm_em_iterate_allreduce(mm_em* em, const double* f, double* f_next, double* ll) {
  if (!em || !f || !f_next || !ll) return MM_ERR_ARG;
  return guarded(em->ctx, [&] { mm::em_iterate_allreduce(em, f, f_next, ll); });
}
int mm_em_run(mm_em* em, const double* f0, int max_iter, double* f_out, double* ll_trace, int ll_cap, int* n_iter) {
  if (!em || !f0 || max_iter <= 0 || !n_iter) return MM_ERR_ARG;
  return guarded(em->ctx, [&] { *n_iter = mm::em_run(em, f0, max_iter, f_out, ll_trace, ll_cap, nullptr); });
}
int mm_em_continue(mm_em* em, int max_iter, double* f_out, double* ll_trace, int ll_cap, int* n_iter, int* stopped) {
  if (!em || max_iter <= 0 || !n_iter) return MM_ERR_ARG;
  return guarded(em->ctx, [&] {
    bool st = false;
    *n_iter = mm::em_run(em, nullptr, max_iter, f_out, ll_trace, ll_cap, &st);
    if (stopped) *stopped = st ? 1 : 0;
  });
}
int mm_em_posteriors(mm_em* em, const double* f, double* post, int64_t* best) {
  if (!em || !f) return MM_ERR_ARG;
  return guarded(em->ctx, [&] { mm::em_posteriors(em, f, post, best); });
}
int mm_em_bootstrap(mm_em* em, const double* f_start, int32_t rep0, int32_t n_rep, uint64_t seed, const uint8_t* weights,
                    int max_iter, double* f_out, double* ll_out, int32_t* n_iter, int32_t* stopped) {
  if (!em || !f_start || n_rep <= 0 || rep0 < 0 || (int64_t)rep0 + n_rep - 1 > INT32_MAX || max_iter <= 0 || !f_out || !ll_out || !n_iter || !stopped) return MM_ERR_ARG;
  return guarded(em->ctx, [&] { mm::boot_run(em, f_start, rep0, n_rep, seed, weights, max_iter, f_out, ll_out, n_iter, stopped); });
}
int mm_em_lca(mm_em* em, const double* f, int32_t n_nodes, const int32_t* parent, const int32_t* taxon_node, double threshold,
              int32_t* node_out, double* mass_out, int64_t* direct_out) {
  if (!em || !f || !parent || !taxon_node || !node_out || n_nodes <= 0) return MM_ERR_ARG;
  return guarded(em->ctx, [&] { mm::lca_run(em, f, n_nodes, parent, taxon_node, threshold, node_out, mass_out, direct_out); });
}
int mm_gene_overlap(mm_ctx* ctx, int32_t n_contigs, const int64_t* contig_gene_off, const int32_t* gene_start, const int32_t* gene_stop,
                    const int32_t* gene_group, int32_t n_groups, const int64_t* group_feat_off, const int32_t* group_feat, int32_t n_feats,
                    int64_t n_maps, const int32_t* map_contig, const int32_t* map_start, const int32_t* map_stop, const double* map_ident,
                    int64_t* group_reads, double* group_median, int64_t* feat_reads, int64_t* maps_on_annotated) {
  if (!ctx) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    MM_REQUIRE(n_contigs >= 0 && n_groups >= 0 && n_feats >= 0 && n_maps >= 0 && contig_gene_off && group_feat_off, MM_ERR_ARG, "mm_gene_overlap: a negative size or no offsets");
    const int64_t ng = n_contigs > 0 ? contig_gene_off[n_contigs] : 0;
    MM_REQUIRE((ng <= 0 || (gene_start && gene_stop && gene_group)) && (n_maps == 0 || (map_contig && map_start && map_stop && map_ident)) &&
               (n_groups == 0 || (group_reads && group_median)) && (group_feat_off[n_groups] <= 0 || group_feat), MM_ERR_ARG, "mm_gene_overlap: a null array");
    mm::gene_overlap_run(ctx, mm::GeneIn{n_contigs, contig_gene_off, gene_start, gene_stop, gene_group, n_groups, group_feat_off, group_feat, n_feats,
                                         n_maps, map_contig, map_start, map_stop, map_ident}, group_reads, group_median, feat_reads, maps_on_annotated);
  });
}
int mm_ident_filter(mm_ctx* ctx, int64_t n_reads, const int64_t* read_off, const int32_t* taxon, const double* ident, const int64_t* best, int32_t n_taxa,
                    double thr_percent, double* sorted_max, int64_t* n_with_entries, int64_t* n_le, int64_t* taxon_reads, double* taxon_median,
                    uint8_t* taxon_removed, uint8_t* read_removed, int64_t* read_src, int64_t* entry_src, int64_t* read_off_out, int64_t* n_reads_out,
                    int64_t* n_entries_out) {
  if (!ctx) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    MM_REQUIRE(n_reads >= 0 && n_taxa >= 0 && read_off && n_with_entries && n_le, MM_ERR_ARG, "mm_ident_filter: a negative size, no offsets or no counts");
    const int n_filtered = (read_src != nullptr) + (entry_src != nullptr) + (read_off_out != nullptr) + (n_reads_out != nullptr) + (n_entries_out != nullptr);
    MM_REQUIRE(n_filtered == 0 || n_filtered == 5, MM_ERR_ARG, "mm_ident_filter: the outputs of the filtered problem are null as a group or not at all");
    MM_REQUIRE((n_reads == 0 || (best && read_removed && sorted_max)) && (read_off[0] != 0 || n_reads == 0 || read_off[n_reads] <= 0 || (taxon && ident)) &&
               (n_taxa == 0 || (taxon_reads && taxon_median && taxon_removed)), MM_ERR_ARG, "mm_ident_filter: a null array");
    mm::ident_filter_run(ctx, mm::IdentIn{n_reads, read_off, taxon, ident, best, n_taxa, thr_percent},
                         mm::IdentOut{sorted_max, n_with_entries, n_le, taxon_reads, taxon_median, taxon_removed, read_removed, read_src, entry_src, read_off_out,
                                      n_reads_out, n_entries_out});
  });
}
int mm_edit_infix(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand,
                  const int32_t* contig, const int64_t* ws, const int64_t* we, const int32_t* max_dist, int32_t* dist_out, int64_t* begin_out, int64_t* end_out) {
  if (!ctx || !reads || !reference) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    require_jobs("mm_edit_infix", n_jobs, read && strand && contig && ws && we && max_dist && dist_out && begin_out && end_out);
    mm::edit_infix_run(ctx, reads, reference, mm::EditInfixIn{n_jobs, read, strand, contig, ws, we, max_dist}, dist_out, begin_out, end_out);
  });
}
int mm_mapping_edit_distances(mm_ctx* ctx, const mm_mapping* mapping, const mm_seqset* reads, const mm_seqset* reference, float perc_identity,
                              int32_t* dist_out, int64_t* first_out, int64_t* last_out, int64_t cap) {
  if (!ctx || !mapping || !reads || !reference) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    require_records("mm_mapping_edit_distances", mapping->n_rec, dist_out && first_out && last_out);
    mm::edit_mapping_run(ctx, mapping, reads, reference, perc_identity, dist_out, first_out, last_out, cap);
  });
}
struct mm_alignment { mm::EditAlignment a; };                      // (host memory only: nothing of the device's outlives the call that made it)
int mm_edit_infix_align(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand,
                        const int32_t* contig, const int64_t* ws, const int64_t* we, const int32_t* max_dist, mm_alignment** out) {
  if (!ctx || !reads || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_alignment& al) {
    require_jobs("mm_edit_infix_align", n_jobs, read && strand && contig && ws && we && max_dist);
    mm::edit_infix_align_run(ctx, reads, reference, mm::EditInfixIn{n_jobs, read, strand, contig, ws, we, max_dist}, &al.a);
  });
}
int mm_mapping_align(mm_ctx* ctx, const mm_mapping* mapping, const mm_seqset* reads, const mm_seqset* reference, float perc_identity, mm_alignment** out) {
  if (!ctx || !mapping || !reads || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_alignment& al) {
    require_records("mm_mapping_align", mapping->n_rec, true);
    mm::edit_mapping_align_run(ctx, mapping, reads, reference, perc_identity, &al.a);
  });
}
int mm_alignment_sizes(const mm_alignment* al, int64_t* n_jobs, int64_t* n_ops) {
  if (!al || !n_jobs || !n_ops) return MM_ERR_ARG;
  *n_jobs = (int64_t)al->a.dist.size(); *n_ops = (int64_t)al->a.ops.size();
  return MM_OK;
}
int mm_alignment_fetch(const mm_alignment* al, int32_t* dist, int64_t* first, int64_t* last, int64_t* op_off, uint32_t* ops) {
  if (!al || !op_off || (!al->a.dist.empty() && (!dist || !first || !last)) || (!al->a.ops.empty() && !ops)) return MM_ERR_ARG;
  const mm::EditAlignment& a = al->a;
  if (!a.dist.empty()) { memcpy(dist, a.dist.data(), a.dist.size() * sizeof(int32_t)); memcpy(first, a.first.data(), a.first.size() * sizeof(int64_t)); memcpy(last, a.last.data(), a.last.size() * sizeof(int64_t)); }
  memcpy(op_off, a.op_off.data(), a.op_off.size() * sizeof(int64_t));
  if (!a.ops.empty()) memcpy(ops, a.ops.data(), a.ops.size() * sizeof(uint32_t));
  return MM_OK;
}
void mm_alignment_destroy(mm_alignment* al) { delete al; }

struct mm_bam { mm::BamMembers b; };                               // (host memory only, as mm_alignment)
int mm_bam_encode(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                  const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint16_t* flag, const uint8_t* mapq,
                  const int64_t* name_off, const char* names, int64_t group_bytes, mm_bam** out) {
  if (!ctx || !reads || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_bam& b) {
    require_jobs("mm_bam_encode", n_jobs, read && strand && contig && dist && first && op_off && flag && mapq && name_off);
    mm::bam_encode_run(ctx, reads, reference, mm::AlignedJobsIn{n_jobs, read, strand, contig, dist, first, op_off, ops}, mm::BamColumns{flag, mapq, name_off, names}, group_bytes, false, &b.b);
  });
}
int mm_bam_encode_sorted(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                         const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint16_t* flag, const uint8_t* mapq,
                         const int64_t* name_off, const char* names, int64_t group_bytes, mm_bam** out) {
  if (!ctx || !reads || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_bam& b) {
    require_jobs("mm_bam_encode_sorted", n_jobs, read && strand && contig && dist && first && op_off && flag && mapq && name_off);
    mm::bam_encode_run(ctx, reads, reference, mm::AlignedJobsIn{n_jobs, read, strand, contig, dist, first, op_off, ops}, mm::BamColumns{flag, mapq, name_off, names}, group_bytes, true, &b.b);
  });
}
int mm_bam_fetch_records(const mm_bam* b, int64_t* job, int64_t* raw_off) {
  if (!b || !raw_off || (!b->b.rec_job.empty() && !job)) return MM_ERR_ARG;
  if (!b->b.rec_job.empty()) memcpy(job, b->b.rec_job.data(), b->b.rec_job.size() * sizeof(int64_t));
  memcpy(raw_off, b->b.rec_off.data(), b->b.rec_off.size() * sizeof(int64_t));
  return MM_OK;
}
int mm_bam_sizes(const mm_bam* b, int64_t* n_records, int64_t* raw_bytes, int64_t* bgzf_bytes) {
  if (!b || !n_records || !raw_bytes || !bgzf_bytes) return MM_ERR_ARG;
  *n_records = b->b.n_records; *raw_bytes = b->b.raw_bytes; *bgzf_bytes = (int64_t)b->b.bgzf.size();
  return MM_OK;
}
int mm_bam_fetch(const mm_bam* b, uint8_t* bgzf) {
  if (!b || (!b->b.bgzf.empty() && !bgzf)) return MM_ERR_ARG;
  if (!b->b.bgzf.empty()) memcpy(bgzf, b->b.bgzf.data(), b->b.bgzf.size());
  return MM_OK;
}
void mm_bam_destroy(mm_bam* b) { delete b; }

struct mm_reads_text { mm::ReadsText t; };                         // (host memory only, as mm_bam)
int mm_reads_encode(mm_ctx* ctx, const mm_seqset* reads, int64_t n_sel, const int32_t* read, const int64_t* name_off, const char* names, int with_qual, int64_t group_bytes,
                    mm_reads_text** out) {
  if (!ctx || !reads || !out) return refused(out);
  return created(ctx, out, [&](mm_reads_text& t) {
    MM_REQUIRE(n_sel >= 0 && n_sel < ((int64_t)1 << 31), n_sel < 0 ? MM_ERR_ARG : MM_ERR_LIMIT, "mm_reads_encode: a negative number of records, or 2^31 or more");
    MM_REQUIRE(n_sel == 0 || (read && name_off), MM_ERR_ARG, "mm_reads_encode: a null array");
    MM_REQUIRE(with_qual == 0 || with_qual == 1, MM_ERR_ARG, "mm_reads_encode: with_qual is neither 0 nor 1");
    mm::reads_encode_run(ctx, reads, mm::ReadsSelection{n_sel, read, name_off, names}, with_qual != 0, group_bytes, &t.t);
  });
}
int mm_reads_text_sizes(const mm_reads_text* t, int64_t* n_records, int64_t* raw_bytes, int64_t* bgzf_bytes) {
  if (!t || !n_records || !raw_bytes || !bgzf_bytes) return MM_ERR_ARG;
  *n_records = t->t.n_records; *raw_bytes = t->t.raw_bytes; *bgzf_bytes = (int64_t)t->t.bgzf.size();
  return MM_OK;
}
int mm_reads_text_fetch(const mm_reads_text* t, uint8_t* bgzf) {
  if (!t || (!t->t.bgzf.empty() && !bgzf)) return MM_ERR_ARG;
  if (!t->t.bgzf.empty()) memcpy(bgzf, t->t.bgzf.data(), t->t.bgzf.size());
  return MM_OK;
}
void mm_reads_text_destroy(mm_reads_text* t) { delete t; }

struct mm_bam_sorter { mm_ctx* ctx = nullptr; mm::BamSorter s; };
int mm_bam_sorter_create(mm_ctx* ctx, int32_t n_ref, const int32_t* ref_len, int64_t window_bytes, mm_bam_sorter** out) {
  if (!ctx || !out) return refused(out);
  return created(ctx, out, [&](mm_bam_sorter& h) { mm::bam_sorter_init(h.s, n_ref, ref_len, window_bytes); });
}
void mm_bam_sorter_destroy(mm_bam_sorter* h) { if (h) { bind(h->ctx); delete h; } }
int mm_bam_sorter_add_run(mm_bam_sorter* h, const uint8_t* bgzf, int64_t bgzf_bytes, int64_t n_records, const int64_t* raw_off, const int32_t* ref_id, const int32_t* pos,
                          const int32_t* end) {
  if (!h) return MM_ERR_ARG;
  return guarded(h->ctx, [&] { mm::bam_sorter_add_run(h->s, bgzf, bgzf_bytes, n_records, raw_off, ref_id, pos, end); });
}
int mm_bam_sorter_plan(mm_bam_sorter* h, int64_t* n_windows, int64_t* stream_bytes) {
  if (!h || !n_windows || !stream_bytes) return MM_ERR_ARG;
  return guarded(h->ctx, [&] { mm::bam_sorter_plan(h->ctx, h->s); *n_windows = mm::bam_sorter_windows(h->s); *stream_bytes = h->s.stream_bytes; });
}
int mm_bam_sorter_window(mm_bam_sorter* h, int64_t w, int64_t* bgzf_bytes) {
  if (!h || !bgzf_bytes) return MM_ERR_ARG;
  return guarded(h->ctx, [&] { mm::bam_sorter_window(h->ctx, h->s, w); *bgzf_bytes = (int64_t)h->s.product.size(); });
}
int mm_bam_sorter_index(mm_bam_sorter* h, int64_t header_bytes, int64_t* bai_bytes) {
  if (!h || !bai_bytes) return MM_ERR_ARG;
  return guarded(h->ctx, [&] { mm::bam_sorter_index(h->ctx, h->s, header_bytes); *bai_bytes = (int64_t)h->s.product.size(); });
}
int mm_bam_sorter_fetch(const mm_bam_sorter* h, uint8_t* out) {
  if (!h || (!h->s.product.empty() && !out)) return MM_ERR_ARG;
  if (!h->s.product.empty()) memcpy(out, h->s.product.data(), h->s.product.size());
  return MM_OK;
}

struct mm_pileup : key_table<false> {};
struct mm_pileup_result { mm::PileupResult r; };
int mm_pileup_events_q(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                       const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use, int32_t min_base_quality, mm_pileup** out) {
  return table_events("mm_pileup_events", mm::pileup_events_run, ctx, reads, reference, {n_jobs, read, strand, contig, dist, first, op_off, ops}, use, min_base_quality, out);
}
int mm_pileup_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                     const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use, mm_pileup** out) {
  return mm_pileup_events_q(ctx, reads, reference, n_jobs, read, strand, contig, dist, first, op_off, ops, use, 0, out);
}
int mm_pileup_merge(mm_ctx* ctx, int64_t n, const uint64_t* keys, const uint32_t* counts, mm_pileup** out) {
  return table_merge("mm_pileup_merge", "pairs", "MM_PILEUP_TIMING", ctx, n, keys, nullptr, counts, out);
}
int mm_pileup_sizes(const mm_pileup* t, int64_t* n_pairs) { return table_sizes(t, n_pairs); }
int mm_pileup_fetch(const mm_pileup* t, uint64_t* keys, uint32_t* counts) { return table_fetch(t, keys, nullptr, counts); }
void mm_pileup_destroy(mm_pileup* t) { delete t; }
int mm_pileup_finish(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* keys, const uint32_t* counts, int64_t n_iv, const int32_t* iv_contig,
                     const int64_t* iv_first, const int64_t* iv_last, int64_t min_count, double min_frac, mm_pileup_result** out) {
  if (!ctx || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_pileup_result& r) {
    require_finish("mm_pileup_finish", n, n_iv, keys && counts, iv_contig && iv_first && iv_last);
    mm::pileup_finish_run(ctx, reference, mm::FinishIn{n, keys, nullptr, counts, n_iv, iv_contig, iv_first, iv_last, min_count, min_frac}, &r.r);
  });
}
int mm_pileup_result_sizes(const mm_pileup_result* r, int64_t* n_sites, int64_t* n_contigs) {
  if (!r || !n_sites || !n_contigs) return MM_ERR_ARG;
  *n_sites = (int64_t)r->r.w0.size(); *n_contigs = (int64_t)r->r.alignments.size();
  return MM_OK;
}
int mm_pileup_result_fetch_sites(const mm_pileup_result* r, uint64_t* key, uint32_t* count, uint32_t* depth, uint8_t* ref_byte) {
  if (!r || (!r->r.w0.empty() && (!key || !count || !depth || !ref_byte))) return MM_ERR_ARG;
  const size_t k = r->r.w0.size();
  if (k) { memcpy(key, r->r.w0.data(), k * 8); memcpy(count, r->r.count.data(), k * 4); memcpy(depth, r->r.depth.data(), k * 4); memcpy(ref_byte, r->r.ref_byte.data(), k); }
  return MM_OK;
}
int mm_pileup_result_fetch_contigs(const mm_pileup_result* r, int64_t* alignments, int64_t* covered, int64_t* sum_depth) {
  if (!r || (!r->r.alignments.empty() && (!alignments || !covered || !sum_depth))) return MM_ERR_ARG;
  const size_t k = r->r.alignments.size();
  if (k) { memcpy(alignments, r->r.alignments.data(), k * 8); memcpy(covered, r->r.covered.data(), k * 8); memcpy(sum_depth, r->r.sum_depth.data(), k * 8); }
  return MM_OK;
}
void mm_pileup_result_destroy(mm_pileup_result* r) { delete r; }

struct mm_mod : key_table<false> {};
struct mm_mod_result { mm::ModResult r; };
int mm_mod_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                  const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use, int32_t min_ml, mm_mod** out) {
  return table_events("mm_mod_events", mm::mod_events_run, ctx, reads, reference, {n_jobs, read, strand, contig, dist, first, op_off, ops}, use, min_ml, out);
}
int mm_mod_merge(mm_ctx* ctx, int64_t n, const uint64_t* keys, const uint32_t* counts, mm_mod** out) {
  return table_merge("mm_mod_merge", "pairs", "MM_MODS_TIMING", ctx, n, keys, nullptr, counts, out);
}
int mm_mod_sizes(const mm_mod* t, int64_t* n_pairs) { return table_sizes(t, n_pairs); }
int mm_mod_fetch(const mm_mod* t, uint64_t* keys, uint32_t* counts) { return table_fetch(t, keys, nullptr, counts); }
void mm_mod_destroy(mm_mod* t) { delete t; }
int mm_mod_finish(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* keys, const uint32_t* counts, int32_t n_codes, const uint8_t* code_base, int64_t min_coverage,
                  mm_mod_result** out) {
  if (!ctx || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_mod_result& r) {
    require_rows("mm_mod_finish", "entries", n, keys && counts);
    mm::mod_finish_run(ctx, reference, n, keys, counts, n_codes, code_base, min_coverage, &r.r);
  });
}
int mm_mod_result_sizes(const mm_mod_result* r, int64_t* n_rows) {
  if (!r || !n_rows) return MM_ERR_ARG;
  *n_rows = (int64_t)r->r.site.size();
  return MM_OK;
}
int mm_mod_result_fetch(const mm_mod_result* r, uint64_t* site, uint64_t* n_mod, uint64_t* n_canonical, uint64_t* n_other, uint64_t* n_fail) {
  if (!r) return MM_ERR_ARG;
  const size_t k = r->r.site.size();
  if (k && (!site || !n_mod || !n_canonical || !n_other || !n_fail)) return MM_ERR_ARG;
  if (k) {
    memcpy(site, r->r.site.data(), k * 8); memcpy(n_mod, r->r.n_mod.data(), k * 8); memcpy(n_canonical, r->r.n_canonical.data(), k * 8);
    memcpy(n_other, r->r.n_other.data(), k * 8); memcpy(n_fail, r->r.n_fail.data(), k * 8);
  }
  return MM_OK;
}
void mm_mod_result_destroy(mm_mod_result* r) { delete r; }

struct mm_motif_result { mm::MotifResult r; };                     // (host memory only: one group's rows and sums)
static_assert(MM_MOTIF_SUMS == mmt::SUMS, "the header's sums are the definition's");
int mm_mod_motifs(mm_ctx* ctx, const mm_seqset* reference, int32_t contig_lo, int32_t contig_hi, int64_t n, const uint64_t* keys, const uint32_t* counts, int32_t n_codes,
                  const uint8_t* code_base, int32_t n_motifs, const int32_t* motif_off, const uint8_t* motif_mask, const int32_t* motif_pos, int64_t min_coverage, double min_frac,
                  int32_t combine_strands, mm_motif_result** out) {
  if (!ctx || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_motif_result& r) {
    require_rows("mm_mod_motifs", "entries", n, keys && counts);
    mm::mod_motifs_run(ctx, reference, mm::MotifIn{contig_lo, contig_hi, n, keys, counts, n_codes, code_base, n_motifs, motif_off, motif_mask, motif_pos, min_coverage, min_frac,
                                                   combine_strands}, &r.r);
  });
}
int mm_motif_result_sizes(const mm_motif_result* r, int64_t* n_rows, int64_t* n_summary) {
  if (!r || !n_rows || !n_summary) return MM_ERR_ARG;
  *n_rows = (int64_t)r->r.site.size(); *n_summary = (int64_t)r->r.s_contig.size();
  return MM_OK;
}
int mm_motif_result_fetch_rows(const mm_motif_result* r, uint64_t* site, int32_t* motif, int32_t* code, uint64_t* n_mod, uint64_t* n_canonical, uint64_t* n_other, uint64_t* n_fail) {
  if (!r) return MM_ERR_ARG;
  const size_t k = r->r.site.size();
  if (k && (!site || !motif || !code || !n_mod || !n_canonical || !n_other || !n_fail)) return MM_ERR_ARG;
  if (k) {
    memcpy(site, r->r.site.data(), k * 8); memcpy(motif, r->r.motif.data(), k * 4); memcpy(code, r->r.code.data(), k * 4); memcpy(n_mod, r->r.n_mod.data(), k * 8);
    memcpy(n_canonical, r->r.n_canonical.data(), k * 8); memcpy(n_other, r->r.n_other.data(), k * 8); memcpy(n_fail, r->r.n_fail.data(), k * 8);
  }
  return MM_OK;
}
int mm_motif_result_fetch_summary(const mm_motif_result* r, int32_t* contig, int32_t* motif, int32_t* code, int64_t* sums) {
  if (!r) return MM_ERR_ARG;
  const size_t k = r->r.s_contig.size();
  if (k && (!contig || !motif || !code || !sums)) return MM_ERR_ARG;
  if (k) { memcpy(contig, r->r.s_contig.data(), k * 4); memcpy(motif, r->r.s_motif.data(), k * 4); memcpy(code, r->r.s_code.data(), k * 4); memcpy(sums, r->r.sums.data(), k * MM_MOTIF_SUMS * 8); }
  return MM_OK;
}
void mm_motif_result_destroy(mm_motif_result* r) { delete r; }

struct mm_vcf : key_table<true> {};
struct mm_vcf_result { mm::VcfResult r; };
int mm_vcf_events_q(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                    const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use, int32_t min_base_quality, mm_vcf** out) {
  return table_events("mm_vcf_events", mm::vcf_events_run, ctx, reads, reference, {n_jobs, read, strand, contig, dist, first, op_off, ops}, use, min_base_quality, out);
}
int mm_vcf_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                  const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use, mm_vcf** out) {
  return mm_vcf_events_q(ctx, reads, reference, n_jobs, read, strand, contig, dist, first, op_off, ops, use, 0, out);
}
int mm_vcf_merge(mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, mm_vcf** out) {
  return table_merge("mm_vcf_merge", "triples", "MM_VCF_TIMING", ctx, n, w0, w1, counts, out);
}
int mm_vcf_sizes(const mm_vcf* t, int64_t* n_triples) { return table_sizes(t, n_triples); }
int mm_vcf_fetch(const mm_vcf* t, uint64_t* w0, uint64_t* w1, uint32_t* counts) { return table_fetch(t, w0, w1, counts); }
void mm_vcf_destroy(mm_vcf* t) { delete t; }
int mm_vcf_finish(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, int64_t n_iv, const int32_t* iv_contig,
                  const int64_t* iv_first, const int64_t* iv_last, int64_t min_count, double min_frac, mm_vcf_result** out) {
  if (!ctx || !reference || !out) return refused(out);
  return created(ctx, out, [&](mm_vcf_result& r) {
    require_finish("mm_vcf_finish", n, n_iv, w0 && w1 && counts, iv_contig && iv_first && iv_last);
    mm::vcf_finish_run(ctx, reference, mm::FinishIn{n, w0, w1, counts, n_iv, iv_contig, iv_first, iv_last, min_count, min_frac}, &r.r);
  });
}
int mm_vcf_result_sizes(const mm_vcf_result* r, int64_t* n_alleles) {
  if (!r || !n_alleles) return MM_ERR_ARG;
  *n_alleles = (int64_t)r->r.w0.size();
  return MM_OK;
}
int mm_vcf_result_fetch(const mm_vcf_result* r, uint64_t* w0, uint64_t* w1, uint32_t* count, uint32_t* depth, uint8_t* window) {
  if (!r || (!r->r.w0.empty() && (!w0 || !w1 || !count || !depth || !window))) return MM_ERR_ARG;
  const size_t k = r->r.w0.size();
  if (k) { memcpy(w0, r->r.w0.data(), k * 8); memcpy(w1, r->r.w1.data(), k * 8); memcpy(count, r->r.count.data(), k * 4); memcpy(depth, r->r.depth.data(), k * 4); }
  if (k) memcpy(window, r->r.window.data(), r->r.window.size());
  return MM_OK;
}
void mm_vcf_result_destroy(mm_vcf_result* r) { delete r; }

struct mm_consensus { mm::ConsResult r; };                         // (host memory only: one group's counters and text)
static_assert(MM_CONS_STATS == mmc::STATS, "the header's counters are the definition's");
int mm_consensus(mm_ctx* ctx, const mm_seqset* reference, int32_t contig_lo, int32_t contig_hi, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, int64_t n_iv,
                 const int32_t* iv_contig, const int64_t* iv_first, const int64_t* iv_last, int64_t min_depth, double min_frac, double min_called, int32_t line_width,
                 struct mm_consensus** out) {
  if (!ctx || !reference || !out) return refused(out);
  return created(ctx, out, [&](struct mm_consensus& r) {
    require_finish("mm_consensus", n, n_iv, w0 && w1 && counts, iv_contig && iv_first && iv_last);
    mm::consensus_run(ctx, reference, mm::ConsIn{contig_lo, contig_hi, mm::FinishIn{n, w0, w1, counts, n_iv, iv_contig, iv_first, iv_last, 1, min_frac}, min_depth, min_called, line_width},
                      &r.r);
  });
}
int mm_consensus_sizes(const struct mm_consensus* r, int64_t* n_contigs, int64_t* n_written, int64_t* text_bytes) {
  if (!r || !n_contigs || !n_written || !text_bytes) return MM_ERR_ARG;
  *n_contigs = (int64_t)r->r.contig.size(); *n_written = (int64_t)r->r.written.size(); *text_bytes = (int64_t)r->r.text.size();
  return MM_OK;
}
int mm_consensus_fetch_contigs(const struct mm_consensus* r, int32_t* contig, int64_t* stats) {
  if (!r || (!r->r.contig.empty() && (!contig || !stats))) return MM_ERR_ARG;
  const size_t k = r->r.contig.size();
  if (k) { memcpy(contig, r->r.contig.data(), k * 4); memcpy(stats, r->r.stats.data(), k * MM_CONS_STATS * 8); }
  return MM_OK;
}
int mm_consensus_fetch_text(const struct mm_consensus* r, int32_t* contig, int64_t* text_off, uint8_t* text) {
  if (!r || !text_off || (!r->r.written.empty() && (!contig || !text))) return MM_ERR_ARG;
  const size_t k = r->r.written.size();
  memcpy(text_off, r->r.text_off.data(), (k + 1) * 8);
  if (k) { memcpy(contig, r->r.written.data(), k * 4); memcpy(text, r->r.text.data(), r->r.text.size()); }
  return MM_OK;
}
void mm_consensus_destroy(struct mm_consensus* r) { delete r; }

struct mm_depth { mm::DepthResult r; };                            // (host memory only: runs, counters and windows)
static_assert(MM_DEPTH_STATS == mmdp::STATS, "the header's counters are the definition's");
int mm_depth_profile(mm_ctx* ctx, int64_t n_contigs, const int64_t* contig_len, int64_t n_iv, const int32_t* iv_contig, const int64_t* iv_first, const int64_t* iv_last, int64_t window,
                     int32_t n_thresholds, const int64_t* thresholds, mm_depth** out) {
  if (!ctx || !out) return refused(out);
  return created(ctx, out, [&](mm_depth& r) {
    mm::depth_profile_run(ctx, mm::DepthIn{n_contigs, contig_len, n_iv, iv_contig, iv_first, iv_last, window, n_thresholds, thresholds}, &r.r);
  });
}
int mm_depth_sizes(const mm_depth* r, int64_t* n_runs, int64_t* n_contigs, int64_t* n_windows) {
  if (!r || !n_runs || !n_contigs || !n_windows) return MM_ERR_ARG;
  *n_runs = (int64_t)r->r.run_contig.size(); *n_contigs = (int64_t)r->r.contig.size(); *n_windows = (int64_t)r->r.win_sum.size();
  return MM_OK;
}
int mm_depth_fetch_runs(const mm_depth* r, int32_t* contig, int64_t* start, int64_t* end, uint32_t* depth) {
  if (!r || (!r->r.run_contig.empty() && (!contig || !start || !end || !depth))) return MM_ERR_ARG;
  const size_t k = r->r.run_contig.size();
  if (k) { memcpy(contig, r->r.run_contig.data(), k * 4); memcpy(start, r->r.run_start.data(), k * 8); memcpy(end, r->r.run_end.data(), k * 8); memcpy(depth, r->r.run_depth.data(), k * 4); }
  return MM_OK;
}
int mm_depth_fetch_contigs(const mm_depth* r, int32_t* contig, int64_t* win_off, int64_t* stats) {
  if (!r || !win_off || (!r->r.contig.empty() && (!contig || !stats))) return MM_ERR_ARG;
  const size_t k = r->r.contig.size();
  memcpy(win_off, r->r.win_off.data(), (k + 1) * 8);
  if (k) { memcpy(contig, r->r.contig.data(), k * 4); memcpy(stats, r->r.stats.data(), r->r.stats.size() * 8); }
  return MM_OK;
}
int mm_depth_fetch_windows(const mm_depth* r, int64_t* sum, int64_t* covered) {
  if (!r || (!r->r.win_sum.empty() && (!sum || !covered))) return MM_ERR_ARG;
  const size_t k = r->r.win_sum.size();
  if (k) { memcpy(sum, r->r.win_sum.data(), k * 8); memcpy(covered, r->r.win_covered.data(), k * 8); }
  return MM_OK;
}
void mm_depth_destroy(mm_depth* r) { delete r; }

struct mm_errprof { mm::ErrprofResult r; };                        // (host memory only: the listed contigs and their rows)
static_assert(MM_ERRPROF_COUNTERS == mmep::COUNTERS && MM_ERRPROF_COLS == mmep::COLS && MM_ERRPROF_STATS == mmep::STATS, "the header's constants are the definition's");
int mm_errprof_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand, const int32_t* contig,
                      const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use, uint64_t* counters, int32_t* cols, uint64_t* ident_key) {
  if (!ctx || !reads || !reference) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    require_jobs("mm_errprof_events", n_jobs, read && strand && contig && dist && first && op_off && use && cols && ident_key);
    MM_REQUIRE(counters, MM_ERR_ARG, "mm_errprof_events: a null array");
    mm::errprof_events_run(ctx, reads, reference, mm::AlignedJobsIn{n_jobs, read, strand, contig, dist, first, op_off, ops}, use, counters, cols, ident_key);
  });
}
int mm_errprof_finish(mm_ctx* ctx, int64_t n_contigs, int64_t n, const uint64_t* ident_key, const int32_t* cols, mm_errprof** out) {
  if (!ctx || !out) return refused(out);
  return created(ctx, out, [&](mm_errprof& r) {
    require_rows("mm_errprof_finish", "entries", n, ident_key && cols);
    mm::errprof_finish_run(ctx, n_contigs, n, ident_key, cols, &r.r);
  });
}
int mm_errprof_sizes(const mm_errprof* r, int64_t* n_contigs) {
  if (!r || !n_contigs) return MM_ERR_ARG;
  *n_contigs = (int64_t)r->r.contig.size();
  return MM_OK;
}
int mm_errprof_fetch(const mm_errprof* r, int32_t* contig, int64_t* stats) {
  if (!r || !stats || (!r->r.contig.empty() && !contig)) return MM_ERR_ARG;
  if (!r->r.contig.empty()) memcpy(contig, r->r.contig.data(), r->r.contig.size() * 4);
  memcpy(stats, r->r.stats.data(), r->r.stats.size() * 8);
  return MM_OK;
}
void mm_errprof_destroy(mm_errprof* r) { delete r; }

// ---- communicator -------------------------------------------------------------------------------------
int mm_comm_unique_id(char id[MM_COMM_ID_BYTES]) {
  if (!id) return MM_ERR_ARG;
  return guarded(nullptr, [&] { mm::comm_unique_id(id); });
}
int mm_comm_init(mm_ctx* ctx, const char id[MM_COMM_ID_BYTES], int rank, int nranks) {
  if (!ctx || !id || rank < 0 || rank >= nranks) return MM_ERR_ARG;
  return guarded(ctx, [&] { mm::comm_init(ctx, id, rank, nranks); });
}
int mm_comm_info(mm_ctx* ctx, int* n_ranks, int* rank) {
  if (!ctx) return MM_ERR_ARG;
  return guarded(ctx, [&] { mm::comm_info(ctx, n_ranks, rank); });
}
int mm_comm_share(mm_ctx* ctx, mm_ctx* owner) {
  if (!ctx || !owner || ctx == owner) return MM_ERR_ARG;
  return guarded(ctx, [&] {
    MM_REQUIRE(ctx->comm == nullptr, MM_ERR_STATE, "communicator already initialised");
    MM_REQUIRE(owner->comm != nullptr && !owner->comm_shared && owner->device == ctx->device, MM_ERR_ARG, "mm_comm_share: the owner must hold a communicator on the same device");
    ctx->comm = owner->comm; ctx->comm_shared = true; ctx->comm_rank = owner->comm_rank; ctx->comm_size = owner->comm_size;
  });
}
int mm_comm_allreduce_f64(mm_ctx* ctx, double* host_inout, int64_t n) {
  if (!ctx || (!host_inout && n > 0)) return MM_ERR_ARG;
  return guarded(ctx, [&] { mm::comm_allreduce_f64(ctx, host_inout, n); });
}
void mm_comm_destroy(mm_ctx* ctx) { if (ctx) mm::comm_destroy(ctx); }

}  // extern "C"
