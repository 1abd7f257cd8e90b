// Exact edit distances of mappings on the device (mapDirectly --edit-distance; not in the reference; DESIGN.md section 1, "Edit distances"; the
// definition: mm_edit_core.hpp; the recurrence, its 64-lane schedule and the driver of a pass: mm_edit_bv_core.hpp, the text the host tests run).
//   jobs      (read, strand, contig, ws, we, max_dist), 32-bit each, in device arrays: uploaded after edit_job_check (mm_edit_infix), or written by
//             edit_jobs_kernel from the mapping's records with the window and cap rules (mm_mapping_edit_distances)
//   align     edit_bv_kernel<BT>: one job per wavefront, a workgroup is one wavefront, the job is blockIdx.x (plus the launch's first job).  Per job a
//             bounded prologue narrows the sets' exception runs to the ones inside the read and the window (binary searches with a fixed number of
//             rounds); bv_align then runs pass 1 and pass 2.  A lane's Pv / Mv are registers (BT of them each, the class of the read's blocks per
//             lane: 1 2 4 8 16 32), Peq is in LDS (BT KiB at most, sized per launch from the longest read of the class), the window's symbols
//             come straight from the packed set, 64 columns at a time.  There is no job counter, no atomic, no barrier (a lane reads only the LDS
//             words it wrote), no loop whose trip count depends on the strings.
//   classes   one launch per class that the read set can need, over all jobs: a wavefront whose job is of another class returns at once
//   trace     (mm_edit_infix_align, mm_mapping_align only; mm_edit_trace_core.hpp) edit_trace_kernel<BT>: one aligned job per wavefront, the same classes,
//             prologue and symbol fetch.  Pass 3 stores two words per block and column into the job's part of the launch's scratch, one barrier makes
//             them visible, the walk reads them back in strips and lane 0 writes the runs into the job's slot of 2 d + 1 words.  The host reads d, a,
//             b back, cuts the jobs into launches whose scratch fits the budget (bv_trace_plan; MM_EDIT_TRACE_MB, else an eighth of the free memory)
//             and launches the classes each cut needs.  A scan of the run counts and edit_gather_kernel pack the runs densely.
// An exception run holds a byte other than A C G T (mm_seq.hip upper-cases before it packs), so a base inside a run matches nothing and every
// other base is its 2-bit code: lower case needs no care here.
#include "mm_edit.hpp"
#include "mm_edit_trace_core.hpp"
#include "mm_edit_seq.hpp"
#include "mm_prims.hpp"

namespace mm {


struct EditJobs {
  const int32_t* read; const int32_t* strand; const int32_t* contig; const int32_t* ws; const int32_t* we; const int32_t* max_dist;
  int32_t* dist; int32_t* a; int32_t* b; int64_t n;
};

struct BvWaveLanes {                                              // one lane per thread of a 64-thread workgroup
  static constexpr int HELD = 1;
  __device__ int lane(int) const { return (int)threadIdx.x; }
  template <class T> __device__ void up(const T* v, T* o) const { o[0] = __shfl_up(v[0], 1); }
  template <class T> __device__ T pick(const T* v, int l) const { return __shfl(v[0], l); }
};

template <int BT> __global__ void __launch_bounds__(BV_LANES) edit_bv_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len,
                                                                            EditSeq R, const uint64_t* __restrict__ r_base, EditJobs J, int64_t job0) {
  extern __shared__ uint32_t edit_peq[];
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  const int32_t read = J.read[job];
  if (read < 0) return;                                           // (a record that edit_jobs_kernel refused)
  const int32_t m = q_len[read];
  if (m > EDIT_MAX_READ || bv_class(bv_per_lane(m)) != BT) return;   // too long: stays not aligned; another class: that launch's
  const int32_t ws = J.ws[job], n = J.we[job] - ws;
  const uint64_t qg = q_base[read], rg = r_base[J.contig[job]] + (uint64_t)ws;
  int32_t d, a, b;
  bv_align<BT>(BvWaveLanes{}, Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg, m, J.strand[job], R.narrowed(rg, rg + (uint64_t)n), (int64_t)rg, n, J.max_dist[job], edit_peq, &d, &a, &b);
  if (threadIdx.x == 0) { J.dist[job] = d; J.a[job] = d < 0 ? -1 : a; J.b[job] = d < 0 ? -1 : b; }
}

struct BvTraceWaveLanes : BvWaveLanes { __device__ void sync() const { __syncthreads(); } };

struct EditTrace { const int64_t* scr_off; const int64_t* slot_off; uint32_t* scratch; uint32_t* slots; int32_t* n_runs; };

// the jobs [job0, job1) of one launch; a job that is not aligned, has an empty read or is of another class: nothing (its n_runs stays 0)
template <int BT> __global__ void __launch_bounds__(BV_LANES) edit_trace_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len,
                                                                               EditSeq R, const uint64_t* __restrict__ r_base, EditJobs J, EditTrace T, int64_t job0, int64_t job1) {
  extern __shared__ uint32_t edit_peq[];
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= job1) return;
  const int32_t read = J.read[job];
  if (read < 0) return;
  const int32_t m = q_len[read], d = J.dist[job];
  if (d < 0 || m <= 0 || m > EDIT_MAX_READ || bv_class(bv_per_lane(m)) != BT) return;
  const int32_t a = J.a[job], n = J.b[job] - a;
  const uint64_t qg = q_base[read], rg = r_base[J.contig[job]] + (uint64_t)J.ws[job] + (uint64_t)a;
  const int64_t count = bv_trace<BT>(BvTraceWaveLanes{}, Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg, m, J.strand[job], R.narrowed(rg, rg + (uint64_t)n), (int64_t)rg, n, d,
                                     edit_peq, T.scratch + T.scr_off[job], T.slots + T.slot_off[job]);
  if (threadIdx.x == 0) T.n_runs[job] = (int32_t)(count < bv_trace_slot(d) ? count : bv_trace_slot(d));
}
// the runs of job0 + blockIdx.x from its slot to their place in the dense array
__global__ void __launch_bounds__(BV_LANES) edit_gather_kernel(EditTrace T, const int64_t* __restrict__ op_off, uint32_t* __restrict__ ops, int64_t job0, int64_t n) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= n) return;
  const uint32_t* src = T.slots + T.slot_off[job];
  uint32_t* dst = ops + op_off[job];
  for (int32_t k = (int32_t)threadIdx.x; k < T.n_runs[job]; k += BV_LANES) dst[k] = src[k];
}

struct EditRecArgs {
  const mm_map_record* rec; int64_t n; const int32_t* q_len; int64_t n_reads; const int32_t* r_len; int64_t n_contigs; float pi;
  int32_t* read; int32_t* strand; int32_t* contig; int32_t* ws; int32_t* we; int32_t* max_dist; int32_t* bad;
};
__global__ void __launch_bounds__(256) edit_jobs_kernel(EditRecArgs A) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const mm_map_record r = A.rec[i];
  const bool ok = r.read >= 0 && r.read < A.n_reads && r.ref_contig >= 0 && r.ref_contig < A.n_contigs && (r.strand == 1 || r.strand == -1);
  int64_t ws = 0, we = 0; int32_t cap = 0;
  if (ok) { const int64_t L = A.q_len[r.read]; edit_window(r.ref_start, L, A.r_len[r.ref_contig], &ws, &we); cap = edit_cap(L, A.pi); }
  else *A.bad = 1;
  A.read[i] = ok ? r.read : -1; A.strand[i] = r.strand; A.contig[i] = ok ? r.ref_contig : 0; A.ws[i] = (int32_t)ws; A.we[i] = (int32_t)we; A.max_dist[i] = cap;
}
// dist, ws + a, ws + b - 1 as the caller's types (-1 -1 -1: not aligned); ws null: a and b as they are
__global__ void __launch_bounds__(256) edit_coords_kernel(EditJobs J, bool contig_coords, int64_t* __restrict__ first, int64_t* __restrict__ last) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= J.n) return;
  const bool al = J.dist[i] >= 0;
  first[i] = !al ? -1 : contig_coords ? (int64_t)J.ws[i] + J.a[i] : J.a[i];
  last[i] = !al ? -1 : contig_coords ? (int64_t)J.ws[i] + J.b[i] - 1 : J.b[i];
}

namespace {

constexpr int EDIT_N_CLASSES = 6;                                 // BT = 1 << c
constexpr int64_t EDIT_GRID_MAX = (int64_t)1 << 30;               // workgroups per launch

struct EditRun {
  mm_ctx* ctx; const mm_seqset* reads; const mm_seqset* ref; hipStream_t st; int64_t n;
  StageClock<3> clk;                                               // MM_EDIT_TIMING=1: jobs, align (and trace) on stderr
  std::string trace_note;                                          // what trace() did, for that line
  DBuf<int32_t> d_read, d_strand, d_contig, d_ws, d_we, d_md, d_dist, d_a, d_b;
  DBuf<int64_t> d_first, d_last;

  EditRun(mm_ctx* c, const mm_seqset* q, const mm_seqset* r, int64_t n_)
      : ctx(c), reads(q), ref(r), st(c->stream), n(n_), clk(getenv("MM_EDIT_TIMING") != nullptr, c->stream) {
    const size_t k = (size_t)std::max<int64_t>(n, 1);
    d_read.alloc(k); d_strand.alloc(k); d_contig.alloc(k); d_ws.alloc(k); d_we.alloc(k); d_md.alloc(k); d_dist.alloc(k); d_a.alloc(k); d_b.alloc(k);
    d_first.alloc(k); d_last.alloc(k);
  }
  EditJobs jobs() const { return EditJobs{d_read.p, d_strand.p, d_contig.p, d_ws.p, d_we.p, d_md.p, d_dist.p, d_a.p, d_b.p, n}; }

  template <int BT> void launch(int32_t B, int64_t job0, int64_t count) {
    const size_t lds = (size_t)bv_peq_words(B) * sizeof(uint32_t);
    edit_bv_kernel<BT><<<dim3((unsigned)count), dim3(BV_LANES), lds, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, edit_seq(ref), ref->d_base.p, jobs(), job0);
    MM_KERNEL_CHECK();
  }
  // every class that a read of the set can need, over all jobs; the LDS of a launch from the longest read of its class
  void align() {
    int32_t B_of[EDIT_N_CLASSES] = {};
    for (const int32_t L : reads->len) {
      if (L > EDIT_MAX_READ) continue;
      const int32_t B = std::max(bv_per_lane(L), 1); int c = 0;      // (an empty read: the first class, no block)
      while ((1 << c) < B) ++c;
      B_of[c] = std::max(B_of[c], B);
    }
    MM_HIP(hipMemsetAsync(d_dist.p, 0xFF, d_dist.bytes(), st)); MM_HIP(hipMemsetAsync(d_a.p, 0xFF, d_a.bytes(), st)); MM_HIP(hipMemsetAsync(d_b.p, 0xFF, d_b.bytes(), st));
    clk.start();
    for (int c = 0; c < EDIT_N_CLASSES; ++c) {
      if (!B_of[c]) continue;
      for (int64_t job0 = 0; job0 < n; job0 += EDIT_GRID_MAX) {
        const int64_t count = std::min(EDIT_GRID_MAX, n - job0);
        switch (c) {
          case 0: launch<1>(B_of[c], job0, count); break;
          case 1: launch<2>(B_of[c], job0, count); break;
          case 2: launch<4>(B_of[c], job0, count); break;
          case 3: launch<8>(B_of[c], job0, count); break;
          case 4: launch<16>(B_of[c], job0, count); break;
          default: launch<32>(B_of[c], job0, count); break;
        }
      }
    }
    clk.stop(1);
  }
  template <int BT> void launch_trace(int32_t B, int64_t job0, int64_t job1, const EditTrace& T) {
    const size_t lds = (size_t)bv_peq_words(B) * sizeof(uint32_t);
    edit_trace_kernel<BT><<<dim3((unsigned)(job1 - job0)), dim3(BV_LANES), lds, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, edit_seq(ref), ref->d_base.p, jobs(), T, job0, job1);
    MM_KERNEL_CHECK();
  }
  // the scratch of one launch in words: MM_EDIT_TRACE_MB, else an eighth of what the device has free now.  Free: what the driver says and what the
  // device's pool of index-scale blocks holds, where the previous call's scratch waits, so that the next call asks for the same size and gets that block
  static int64_t trace_budget_words() {
    if (const char* e = getenv("MM_EDIT_TRACE_MB")) if (atoll(e) > 0) return (int64_t)atoll(e) << 18;
    size_t fr = 0, tot = 0;
    MM_HIP(dev_mem_info(&fr, &tot));
    return (int64_t)((fr + big_pool_bytes(dev_current())) / 8 / sizeof(uint32_t));
  }
  // the runs of every aligned job, after align(): op_off (n + 1) and ops
  void trace(std::vector<int64_t>* op_off, std::vector<uint32_t>* ops) {
    const size_t k = (size_t)n;
    std::vector<int32_t> h_read(k), h_dist(k), h_a(k), h_b(k), m(k);
    d_read.download(h_read.data(), k, st); d_dist.download(h_dist.data(), k, st); d_a.download(h_a.data(), k, st); d_b.download(h_b.data(), k, st);
    MM_HIP(mm::stream_sync(st));
    for (size_t i = 0; i < k; ++i) m[i] = h_read[i] < 0 ? 0 : reads->len[(size_t)h_read[i]];
    const int64_t budget = trace_budget_words();
    const TracePlan P = bv_trace_plan(n, m.data(), h_dist.data(), h_a.data(), h_b.data(), budget, EDIT_GRID_MAX);
    DBuf<int64_t> d_scr_off(k), d_slot_off(k), d_op_off(k + 1);
    DBuf<uint32_t> scratch((size_t)std::max<int64_t>(P.scratch_words, 1)), slots((size_t)std::max<int64_t>(P.slot_words, 1));
    DBuf<int32_t> d_runs(k + 1);
    d_scr_off.upload(P.scr_off.data(), k, st); d_slot_off.upload(P.slot_off.data(), k, st); d_runs.zero(st);
    const EditTrace T{d_scr_off.p, d_slot_off.p, scratch.p, slots.p, d_runs.p};
    clk.start();
    int64_t launches = 0;
    for (size_t c = 0; c + 1 < P.cut.size(); ++c) {
      int32_t B_of[EDIT_N_CLASSES] = {};
      for (int64_t i = P.cut[c]; i < P.cut[c + 1]; ++i) {
        if (!bv_trace_wanted(m[(size_t)i], h_dist[(size_t)i])) continue;
        const int32_t B = bv_per_lane(m[(size_t)i]); int cl = 0;
        while ((1 << cl) < B) ++cl;
        B_of[cl] = std::max(B_of[cl], B);
      }
      for (int cl = 0; cl < EDIT_N_CLASSES; ++cl) {
        if (!B_of[cl]) continue;
        ++launches;
        switch (cl) {
          case 0: launch_trace<1>(B_of[cl], P.cut[c], P.cut[c + 1], T); break;
          case 1: launch_trace<2>(B_of[cl], P.cut[c], P.cut[c + 1], T); break;
          case 2: launch_trace<4>(B_of[cl], P.cut[c], P.cut[c + 1], T); break;
          case 3: launch_trace<8>(B_of[cl], P.cut[c], P.cut[c + 1], T); break;
          case 4: launch_trace<16>(B_of[cl], P.cut[c], P.cut[c + 1], T); break;
          default: launch_trace<32>(B_of[cl], P.cut[c], P.cut[c + 1], T); break;
        }
      }
    }
    DBuf<uint8_t> tmp;
    exclusive_scan(tmp, d_runs.p, d_op_off.p, k + 1, st);
    *op_off = d_op_off.to_host(st);
    const int64_t total = op_off->back();
    DBuf<uint32_t> d_ops((size_t)std::max<int64_t>(total, 1));
    for (int64_t job0 = 0; job0 < n; job0 += EDIT_GRID_MAX) {
      edit_gather_kernel<<<dim3((unsigned)std::min(EDIT_GRID_MAX, n - job0)), dim3(BV_LANES), 0, st>>>(T, d_op_off.p, d_ops.p, job0, n); MM_KERNEL_CHECK();
    }
    clk.stop(2);
    *ops = d_ops.to_host(st, (size_t)total);
    char note[160];
    snprintf(note, sizeof note, " trace %.3f ms; budget %lld MiB, scratch %lld MiB, %lld launches, %lld runs", clk.ms[2], (long long)(budget >> 18), (long long)(P.scratch_words >> 18),
             (long long)launches, (long long)total);
    trace_note = note;
  }
  void fetch(bool contig_coords, int32_t* dist, int64_t* first, int64_t* last) {
    edit_coords_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(jobs(), contig_coords, d_first.p, d_last.p); MM_KERNEL_CHECK();
    d_dist.download(dist, (size_t)n, st); d_first.download(first, (size_t)n, st); d_last.download(last, (size_t)n, st);
    MM_HIP(mm::stream_sync(st));
    if (clk.on) fprintf(stderr, "MM_EDIT_TIMING jobs %.3f align %.3f ms; %lld jobs%s\n", clk.ms[0], clk.ms[1], (long long)n, trace_note.c_str());
  }
};

void edit_sets_check(const mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const char* who) {
  MM_REQUIRE(reads->frozen && ref->frozen, MM_ERR_STATE, std::string(who) + ": a sequence set is not uploaded");
  MM_REQUIRE(reads->ctx->device == ctx->device && ref->ctx->device == ctx->device, MM_ERR_ARG, std::string(who) + ": a sequence set lives on another device");
}

}  // namespace

// every job, before anything is launched; the windows as the kernels take them
static void edit_infix_check(const mm_seqset* reads, const mm_seqset* ref, const EditInfixIn& in, const std::string& who, std::vector<int32_t>& ws, std::vector<int32_t>& we) {
  const size_t n = (size_t)in.n_jobs;
  ws.resize(n); we.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const int bad = edit_job_check(in.read[i], in.strand[i], in.contig[i], in.max_dist[i], in.ws[i], in.we[i], reads->count(), ref->count(), ref->len.data());
    MM_REQUIRE(!bad, MM_ERR_ARG, who + ": " + edit_arg_message(bad));
    ws[i] = (int32_t)in.ws[i]; we[i] = (int32_t)in.we[i];
  }
}
static void edit_infix_upload(EditRun& J, const EditInfixIn& in, const std::vector<int32_t>& ws, const std::vector<int32_t>& we) {
  const size_t n = (size_t)in.n_jobs;
  J.d_read.upload(in.read, n, J.st); J.d_strand.upload(in.strand, n, J.st); J.d_contig.upload(in.contig, n, J.st);
  J.d_ws.upload(ws.data(), n, J.st); J.d_we.upload(we.data(), n, J.st); J.d_md.upload(in.max_dist, n, J.st);
}
// the jobs of a mapping's records, made on the device
static void edit_mapping_jobs(EditRun& J, const mm_mapping* M, const mm_seqset* reads, const mm_seqset* ref, float pi, const std::string& who) {
  DBuf<int32_t> d_bad(1); d_bad.zero(J.st);
  J.clk.start();
  edit_jobs_kernel<<<dim3(flat_grid(J.n)), dim3(256), 0, J.st>>>(EditRecArgs{M->rec.p, J.n, reads->d_len.p, reads->count(), ref->d_len.p, ref->count(), pi,
                                                                             J.d_read.p, J.d_strand.p, J.d_contig.p, J.d_ws.p, J.d_we.p, J.d_md.p, d_bad.p});
  MM_KERNEL_CHECK();
  const int32_t bad = d_bad.to_host(J.st)[0];
  J.clk.stop(0);
  MM_REQUIRE(!bad, MM_ERR_ARG, who + ": a record's read, contig or strand lies outside the sets (is `reference` the set the index was built from?)");
}
static void edit_mapping_check(const mm_ctx* ctx, const mm_mapping* M, const mm_seqset* reads, const mm_seqset* ref, const std::string& who) {
  edit_sets_check(ctx, reads, ref, who.c_str());
  MM_REQUIRE(M->ctx->device == ctx->device, MM_ERR_ARG, who + ": the mapping lives on another device");
  MM_REQUIRE(!M->sketch_only, MM_ERR_STATE, who + ": the mapping has no records");
  MM_REQUIRE(reads->count() == M->n_reads, MM_ERR_ARG, who + ": the read set is not the one that was mapped");
}
static void edit_alignment_size(EditAlignment* out, int64_t n) {
  out->dist.assign((size_t)n, -1); out->first.assign((size_t)n, -1); out->last.assign((size_t)n, -1); out->op_off.assign((size_t)n + 1, 0); out->ops.clear();
}

void edit_infix_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const EditInfixIn& in, int32_t* dist, int64_t* begin, int64_t* end) {
  edit_sets_check(ctx, reads, ref, "mm_edit_infix");
  std::vector<int32_t> ws, we;
  edit_infix_check(reads, ref, in, "mm_edit_infix", ws, we);
  if (in.n_jobs == 0) return;
  EditRun J(ctx, reads, ref, in.n_jobs);
  edit_infix_upload(J, in, ws, we);
  J.align();
  J.fetch(false, dist, begin, end);
}

void edit_mapping_run(mm_ctx* ctx, const mm_mapping* M, const mm_seqset* reads, const mm_seqset* ref, float pi, int32_t* dist, int64_t* first, int64_t* last, int64_t cap) {
  edit_mapping_check(ctx, M, reads, ref, "mm_mapping_edit_distances");
  MM_REQUIRE(cap >= M->n_rec, MM_ERR_ARG, "output capacity too small");
  if (M->n_rec == 0) return;
  EditRun J(ctx, reads, ref, M->n_rec);
  edit_mapping_jobs(J, M, reads, ref, pi, "mm_mapping_edit_distances");
  J.align();
  J.fetch(true, dist, first, last);
}

void edit_infix_align_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const EditInfixIn& in, EditAlignment* out) {
  edit_sets_check(ctx, reads, ref, "mm_edit_infix_align");
  std::vector<int32_t> ws, we;
  edit_infix_check(reads, ref, in, "mm_edit_infix_align", ws, we);
  edit_alignment_size(out, in.n_jobs);
  if (in.n_jobs == 0) return;
  EditRun J(ctx, reads, ref, in.n_jobs);
  edit_infix_upload(J, in, ws, we);
  J.align();
  J.trace(&out->op_off, &out->ops);
  J.fetch(false, out->dist.data(), out->first.data(), out->last.data());
}

void edit_mapping_align_run(mm_ctx* ctx, const mm_mapping* M, const mm_seqset* reads, const mm_seqset* ref, float pi, EditAlignment* out) {
  edit_mapping_check(ctx, M, reads, ref, "mm_mapping_align");
  edit_alignment_size(out, M->n_rec);
  if (M->n_rec == 0) return;
  EditRun J(ctx, reads, ref, M->n_rec);
  edit_mapping_jobs(J, M, reads, ref, pi, "mm_mapping_align");
  J.align();
  J.trace(&out->op_off, &out->ops);
  J.fetch(true, out->dist.data(), out->first.data(), out->last.data());
}

}  // namespace mm
