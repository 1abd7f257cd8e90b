"""What profiles/edit_kernel_stats.txt is made from: mm_mapping_edit_distances on one batch of bench size (10^5 synthetic ONT-error reads of 10 kb against a
uniform synthetic reference, best mappings only) timed stage by stage with events on the context's stream (MM_EDIT_TIMING=1, three calls in a fresh child
process), and csrc/mm_edit_core.hpp's edit_infix_host on one host thread over a sample of the same jobs (tools/edit_host_align.cpp, built with g++ into
tools/_tmp/), which also holds the device's answers against the host's.
Usage: python tools/edit_kernel_stats.py [n_reads] [host sample]      (writes profiles/edit_kernel_stats.txt)
       python tools/edit_kernel_stats.py --align [n_reads]            (writes profiles/edit_trace_stats.txt)
       python tools/edit_kernel_stats.py --bam [n_reads]              (writes profiles/bam_encode_stats.txt)
       python tools/edit_kernel_stats.py --reads-out [n_reads]        (writes profiles/reads_out_stats.txt)
       python tools/edit_kernel_stats.py --bam-sort [n_reads]         (writes profiles/bam_sort_stats.txt)
       python tools/edit_kernel_stats.py --pileup [n_reads]           (writes profiles/pileup_stats.txt)
       python tools/edit_kernel_stats.py --vcf [n_reads]              (writes profiles/vcf_stats.txt)
       python tools/edit_kernel_stats.py --consensus [n_reads]        (writes profiles/consensus_stats.txt)
       python tools/edit_kernel_stats.py --qualities [n_reads] [--min-base-quality Q]   (writes profiles/qual_stats.txt)
       python tools/edit_kernel_stats.py --mods [n_reads]   (writes profiles/mods_stats.txt)
       python tools/edit_kernel_stats.py --depth [n_reads]  (writes profiles/depth_stats.txt)
       python tools/edit_kernel_stats.py --error-profile [n_reads]   (writes profiles/errprof_stats.txt)
--error-profile: the batch through mm_mapping_align, twice through mm_pileup_events (the MM_PILEUP_TIMING stage lines: the comparison) and in the same process
through mm_errprof_events (mm_errprof_core.hpp, mm_errprof.hip) twice at the default number of workgroups and once each at G = 1, 2, 4, 8, 16 and 32 per CU
(MM_ERRPROF_GROUPS; the MM_ERRPROF_TIMING lines have the upload, check, walk and sum stages), every result held equal to the first, then twice through
mm_errprof_finish.  One run is one run.
--mods: the batch fetched to the host and uploaded again without and with seeded modification groups (C+m? and A+a. on every C and A, ML uniform in 0 .. 255,
independent of the bases): the upload's wall time both ways with the staged bytes (the MM_MODS_TIMING plane line), then in the same process mm_pileup_events
and mm_mod_events twice each on the same alignments (the MM_PILEUP_TIMING and MM_MODS_TIMING stage lines), mm_mod_merge and mm_mod_finish with the table's
size.  Synthetic tags say nothing about real methylation.  One run is one run.
--motifs: the run of --mods, and behind its mm_mod_finish in the same process mm_mod_motifs (mm_motif_core.hpp, mm_motif.hip) over the same table with the motifs
GATC:1, CCWGG:1 and CG:0, twice without and twice with combined strands, one call per group of at most 2^28 reference bases: the MM_MODS_TIMING motifs lines (scan,
sites, order and copies), the wall time, rows and sums, beside that run's mm_mod_finish.  Written to profiles/motif_stats.txt.  One run is one run.
--depth: the batch through mm_mapping_edit_distances (the intervals need no traceback), then twice through mm_depth_profile (mm_depth_core.hpp, mm_depth.hip)
at the default window and thresholds and once at W = 1 000 000: the MM_DEPTH_TIMING stage lines, the wall time of each call with its copies, the runs, listed
contigs and windows, beside mm_pileup_finish over an empty table and the same intervals (the MM_PILEUP_TIMING finish line), whose three per-contig sums the
profile must repeat.  One run is one run.
--qualities: the batch fetched to the host and uploaded again as a parser would hand it over, without and with seeded qualities (uniform in 2 .. 40 per base,
independent of the bases): the upload's wall time both ways, then in the same process mm_bam_encode on the set without and with the plane, and
mm_pileup_events_q and mm_vcf_events_q at floor 0 and at Q (default 20) with the rows of both tables at each floor.  Synthetic qualities do not correlate with
the synthetic errors, so the shrinkage of the tables says nothing about real reads.  One run is one run.
--consensus: the run of --vcf, and behind its mm_vcf_finish in the same process mm_consensus (mm_cons_core.hpp, mm_cons.hip) over the same table and intervals
at the default thresholds, one call per group of at most 2^28 reference bases: the MM_CONS_TIMING lines, the wall time, the groups, the contigs written and the
bytes of text, beside that run's mm_vcf_finish.  One run is one run.
--vcf: the run of --pileup, and behind it in the same process the same alignments twice through mm_vcf_events (mm_vcf_core.hpp, mm_vcf.hip) and once through
mm_vcf_merge and mm_vcf_finish at the default thresholds: the MM_VCF_TIMING lines, the wall times, the events, triples and bytes fetched, beside that run's
mm_pileup_events, which is the comparison.  One run is one run.
--pileup: the same batch through mm_mapping_align and mm_bam_encode once each, then twice through mm_pileup_events (every aligned best mapping contributes:
mm_pileup_core.hpp, mm_pileup.hip) and once through mm_pileup_merge and mm_pileup_finish at the default thresholds: the stage times (the MM_PILEUP_TIMING
lines), the wall time of each call with its copies, the pairs of the batch and the bytes fetched, beside that run's align and encode times.  One run is one run.
--bam-sort: the same batch through mm_mapping_align once, twice through mm_bam_encode and twice through mm_bam_encode_sorted (wall times, beside each other), then
as four sorted runs and again as one sorted run through mm_bam_sorter_* (mm_bam_sort.hip): the wall times of the runs' encode, of add_run, plan, every window and
the index, and the bytes; the two splits must give byte-identical members and index.  The MM_BAM_SORT_TIMING lines have every window's inflate, gather and deflate times.  One
run is one run.
--reads-out: the same batch's reads, given seeded qualities, through mm_reads_encode (FASTA and FASTQ records of every read, written and deflated on the device:
mm_reads_out_core.hpp, mm_reads_out.hip) twice each: the upload / size / scan / write / deflate stage times (the MM_READS_OUT_TIMING line) and the wall time of the call,
and in the same process the alternative that needs no new kernel: the same text formatted by one host thread from the batch's arena and handed to mm_bgzf_deflate.

--bam: the same batch through mm_mapping_align once and then twice through mm_bam_encode (the BAM records of these alignments, encoded and deflated on the
device: mm_bam_core.hpp, mm_bam.hip): the upload / size / scan / write / deflate stage times (the MM_BAM_TIMING line), the wall time of the call with its
copies, raw and BGZF bytes, beside the same run's mm_mapping_align time (the MM_EDIT_TIMING line) and the size PREFIX.paf would have.  The members are
inflated on the host and counted against the raw bytes.  One run is one run.
--align: the same batch through mm_mapping_align (the alignments behind the distances: mm_edit_trace_core.hpp) in one child process under one timeout: one
distance-only call as the yardstick, then two aligning calls with their jobs / align / trace stage times, the scratch budget and the launches it led to (the
MM_EDIT_TIMING line), the runs, and the size PREFIX.paf would have for these mappings (reads named read<i>, contigs contig<c>)."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, PI, READ_LEN = 16, 80.0, 10_000


def child(n_reads, n_sample):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    for rep in range(3):
        t0 = time.perf_counter()
        dist, first, last = ctx.mapping_edit_distances(M, reads, ref, PI, n)
        dt = time.perf_counter() - t0
        al = dist >= 0
        print(f"mm_mapping_edit_distances call {rep}: {1e3 * dt:.1f} ms wall with the copies to the host, {n / dt:.0f} jobs/s; {int(al.sum())} of {n} aligned, "
              f"mean distance {float(dist[al].mean()) if al.any() else float('nan'):.1f}, mean aligned length {float((last[al] - first[al] + 1).mean()) if al.any() else float('nan'):.1f}", flush=True)
    pick = np.random.default_rng(1).choice(n, size=min(n_sample, n), replace=False)
    rl, cl = reads.lengths(), ref.lengths()
    lines = []
    for i in pick:
        r = rec[i]
        L, C = int(rl[r["read"]]), int(cl[r["ref_contig"]])
        pad = 64 + L // 16
        ws, we = min(max(0, int(r["ref_start"]) - pad), C), min(C, int(r["ref_start"]) + L + pad)
        we = max(we, ws)
        cap = int(np.floor(1.5 * L * (100.0 - float(np.float32(PI))) / 100.0))
        d, a, b = (int(dist[i]), int(first[i]) - ws, int(last[i]) + 1 - ws) if dist[i] >= 0 else (-1, -1, -1)
        lines.append(f"{int(r['strand'])} {cap} {d} {a} {b} ={reads.fetch(int(r['read']), L).decode()} ={ref.fetch(int(r['ref_contig']), C)[ws:we].decode()}")
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()
    exe = os.path.join(ROOT, "tools", "_tmp", "edit_host_align")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "edit_host_align.cpp")], check=True)
    subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), check=True)


def child_reads_out(n_reads):
    """--reads-out: the batch's reads (re-uploaded as ASCII with seeded qualities, which synthetic reads lack) through mm_reads_encode as FASTA and as FASTQ, twice
    each, and the same text formatted by one host thread from the batch's arena and handed to mm_bgzf_deflate, in the same process"""
    import ctypes as C
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    synth, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    arena, ln = synth.fetch_range(0, synth.count)
    synth.close(); ref.close()
    off = np.zeros(len(ln) + 1, dtype=np.int64); np.cumsum(ln, out=off[1:])
    qual = np.random.default_rng(7).integers(2, 41, size=len(arena), dtype=np.uint8)   # seeded Phred 2..40, independent of the bases
    seqs = [arena[off[i]:off[i + 1]].tobytes() for i in range(len(ln))]
    t0 = time.perf_counter()
    reads = ctx.seqset(seqs, quals=[(qual[off[i]:off[i + 1]] + 33).tobytes() for i in range(len(ln))], qual_offset=33)
    print(f"{len(ln)} reads, {len(arena)} bases with qualities uploaded in {time.perf_counter() - t0:.2f} s (the Python wrapper's loop included)", flush=True)
    names = [b"read%d" % i for i in range(len(ln))]
    sel = np.arange(len(ln), dtype=np.int32)
    got = {}
    for wq in (0, 1):
        for rep in range(2):
            t0 = time.perf_counter()
            data, n_rec, raw = ctx.reads_encode(reads, sel, names, wq)
            dt = time.perf_counter() - t0
            print(f"mm_reads_encode {'FASTQ' if wq else 'FASTA'} call {rep}: {1e3 * dt:.1f} ms wall with the copies (the Python wrapper's own included), {n_rec} records, "
                  f"{raw / 1e6:.1f} MB raw, {len(data) / 1e6:.1f} MB BGZF", flush=True)
        got[wq] = data
    L = capi.lib()
    for wq in (0, 1):
        for rep in range(2):
            t0 = time.perf_counter()
            qc = qual + 33 if wq else None
            parts = []
            for i in range(len(ln)):
                a, b = off[i], off[i + 1]
                if wq:
                    parts += [b"@", names[i], b"\n", arena[a:b].data, b"\n+\n", qc[a:b].data, b"\n"]
                else:
                    parts += [b">", names[i], b"\n", arena[a:b].data, b"\n"]
            text = b"".join(parts)
            t1 = time.perf_counter()
            cap = L.mm_bgzf_deflate_bound(len(text))
            out = np.empty(cap, dtype=np.uint8)
            nbytes, nblocks = C.c_int64(-1), C.c_int32(-1)
            ctx.check(L.mm_bgzf_deflate(ctx.h, text, len(text), out.ctypes.data_as(C.c_void_p), cap, C.byref(nbytes), C.byref(nblocks)))
            t2 = time.perf_counter()
            print(f"host alternative {'FASTQ' if wq else 'FASTA'} call {rep}: format on one host thread {1e3 * (t1 - t0):.1f} ms + mm_bgzf_deflate {1e3 * (t2 - t1):.1f} ms = "
                  f"{1e3 * (t2 - t0):.1f} ms wall, {len(text) / 1e6:.1f} MB raw, {nbytes.value / 1e6:.1f} MB BGZF", flush=True)
        import gzip
        same = gzip.decompress(got[wq]) == text if len(text) < (1 << 28) else None
        print(f"the device's inflated stream equals the host's text: {same if same is not None else 'not compared at this size'}", flush=True)
    reads.close(); ctx.close()


def paf_bytes(dist, first, last, op_off, ops, read, read_len, contig, contig_len):
    """the bytes of PREFIX.paf for these answers with reads named read<i> and contigs contig<c>, and those of its CIGAR text; also holds the runs against
    dist, the read lengths and first / last (X + I + D = d, = + X + I = m, = + X + D = n)"""
    ln, op = (ops >> 4).astype(np.int64), (ops & 15).astype(np.int64)
    al = dist >= 0
    job = np.repeat(np.arange(len(dist)), np.diff(op_off))

    def per_job(v):
        return np.bincount(job, weights=v, minlength=len(dist)).astype(np.int64)[al]

    def digits(v):
        return np.floor(np.log10(np.maximum(v, 1))).astype(np.int64) + 1
    n_eq, n_all = per_job(ln * (op == 7)), per_job(ln)
    assert np.array_equal(n_all - n_eq, dist[al]), "X + I + D bases = d"
    assert np.array_equal(per_job(ln * (op != 2)), read_len[al]), "= + X + I = m"
    assert np.array_equal(per_job(ln * (op != 1)), (last - first + 1)[al]), "= + X + D = n"
    cg = int(per_job(digits(ln) + 1).sum())
    cols = [digits(read[al]) + 4, 2 * digits(read_len[al]), digits(contig[al]) + 6, digits(contig_len[al]), digits(first[al]), digits(last[al] + 1), digits(n_eq), digits(n_all),
            digits(dist[al].astype(np.int64))]
    fixed = 13 + 1 + len("0") + len("+") + len("255") + len("NM:i:") + len("cg:Z:")       # 13 tabs, the newline and the constant fields
    return int(sum(int(c.sum()) for c in cols)) + fixed * int(al.sum()) + cg, cg


def child_align(n_reads):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    t0 = time.perf_counter()
    dist0, first0, last0 = ctx.mapping_edit_distances(M, reads, ref, PI, n)
    print(f"mm_mapping_edit_distances (distance only): {1e3 * (time.perf_counter() - t0):.1f} ms wall with the copies to the host", flush=True)
    for rep in range(2):
        t0 = time.perf_counter()
        dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
        dt = time.perf_counter() - t0
        assert np.array_equal(dist, dist0) and np.array_equal(first, first0) and np.array_equal(last, last0)
        print(f"mm_mapping_align call {rep}: {1e3 * dt:.1f} ms wall with the copies to the host, {n / dt:.0f} jobs/s; {int((dist >= 0).sum())} of {n} aligned, "
              f"{len(ops)} runs ({len(ops) / max(n, 1):.1f} per job, {4 * len(ops) / 1e6:.1f} MB)", flush=True)
    rl, cl = reads.lengths()[rec["read"]].astype(np.int64), ref.lengths()[rec["ref_contig"]].astype(np.int64)
    total, cg = paf_bytes(dist, first, last, op_off, ops, rec["read"].astype(np.int64), rl, rec["ref_contig"].astype(np.int64), cl)
    print(f"PREFIX.paf of these mappings: {total / 1e6:.1f} MB, {cg / 1e6:.1f} MB of it CIGAR text", flush=True)
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()


def child_bam(n_reads):
    import io
    import gzip
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    t0 = time.perf_counter()
    dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
    dt = time.perf_counter() - t0
    print(f"mm_mapping_align: {1e3 * dt:.1f} ms wall with the copies to the host; {int((dist >= 0).sum())} of {n} aligned, {len(ops)} runs ({4 * len(ops) / 1e6:.1f} MB)", flush=True)
    rl, cl = reads.lengths()[rec["read"]].astype(np.int64), ref.lengths()[rec["ref_contig"]].astype(np.int64)
    total, cg = paf_bytes(dist, first, last, op_off, ops, rec["read"].astype(np.int64), rl, rec["ref_contig"].astype(np.int64), cl)
    print(f"PREFIX.paf of these mappings: {total / 1e6:.1f} MB, {cg / 1e6:.1f} MB of it CIGAR text (its formatting on the host is not timed here)", flush=True)
    strand = rec["strand"].astype(np.int32)
    names = [b"read%d" % r for r in rec["read"]]
    args = dict(read=rec["read"], strand=strand, contig=rec["ref_contig"], dist=dist, first=first, op_off=op_off, ops=ops, flag=np.where(strand < 0, 0x10, 0), mapq=np.full(n, 60), names=names)
    for rep in range(2):
        t0 = time.perf_counter()
        data, n_rec, raw = ctx.bam_encode(reads, ref, **args)
        dt = time.perf_counter() - t0
        print(f"mm_bam_encode call {rep}: {1e3 * dt:.1f} ms wall with the copies (the Python wrapper's own included), {n_rec} records, {raw / 1e6:.1f} MB raw, {len(data) / 1e6:.1f} MB BGZF "
              f"({raw / max(n_rec, 1):.0f} B per record raw)", flush=True)
    got = 0
    with gzip.GzipFile(fileobj=io.BytesIO(data)) as z:
        while True:
            piece = z.read(1 << 26)
            if not piece:
                break
            got += len(piece)
    assert got == raw and n_rec == int((dist >= 0).sum()), (got, raw, n_rec)
    print(f"the members inflate to {got} bytes on the host: the raw bytes", flush=True)
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()


def child_bam_sort(n_reads):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
    strand = rec["strand"].astype(np.int32)
    contig = rec["ref_contig"].astype(np.int32)

    def args(a, b):
        return dict(read=rec["read"][a:b], strand=strand[a:b], contig=contig[a:b], dist=dist[a:b], first=first[a:b], op_off=op_off[a:b + 1] - op_off[a], ops=ops[op_off[a]:op_off[b]],
                    flag=np.where(strand[a:b] < 0, 0x10, 0), mapq=np.full(b - a, 60), names=[b"read%d" % r for r in rec["read"][a:b]])
    for name, entry in (("mm_bam_encode", ctx.bam_encode), ("mm_bam_encode_sorted", ctx.bam_encode_sorted)):
        for rep in range(2):
            t0 = time.perf_counter()
            data, n_rec, raw = entry(reads, ref, **args(0, n))
            print(f"{name} call {rep}: {1e3 * (time.perf_counter() - t0):.1f} ms wall with the copies (the Python wrapper's own included), {n_rec} records, {raw / 1e6:.1f} MB raw, "
                  f"{len(data) / 1e6:.1f} MB BGZF", flush=True)
    whole = None
    for n_runs in (4, 1):
        cuts = [n * r // n_runs for r in range(n_runs + 1)]
        t0 = time.perf_counter()
        runs = [(a, ctx.bam_records(reads, ref, sorted=True, **args(a, b))) for a, b in zip(cuts, cuts[1:])]
        t_encode = time.perf_counter() - t0
        S = capi.BamSorter(ctx, ref.lengths())
        t0 = time.perf_counter()
        for a, (data, job, raw_off) in runs:
            pos = first[a + job]
            S.add_run(data, raw_off, contig[a + job], pos, np.maximum(pos + 1, last[a + job] + 1))
        t_add = time.perf_counter() - t0
        t0 = time.perf_counter()
        n_windows, stream = S.plan()
        t_plan = time.perf_counter() - t0
        t_win, out = [], []
        for k in range(n_windows):
            t0 = time.perf_counter()
            out.append(S.window(k))
            t_win.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        bai = S.index(0)
        t_index = time.perf_counter() - t0
        S.close()
        body = b"".join(out)
        assert whole is None or whole == (body, bai)
        whole = (body, bai)
        print(f"{n_runs} run(s): sorted encode {1e3 * t_encode:.1f} ms, add_run {1e3 * t_add:.1f} ms (host: the member chains and the keys' checks), "
              f"plan {1e3 * t_plan:.1f} ms, {n_windows} windows of 255 MiB {1e3 * sum(t_win):.1f} ms ({', '.join(f'{1e3 * t:.0f}' for t in t_win)}; the MM_BAM_SORT_TIMING lines have each window's inflate, gather and deflate), index {1e3 * t_index:.1f} ms; {stream / 1e6:.1f} MB of records -> {len(body) / 1e6:.1f} MB BGZF, "
              f".bai {len(bai)} bytes; wall times with the copies, one run", flush=True)
    print("the files of the two splits are byte-identical", flush=True)
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()


def child_pileup(n_reads, vcf=False, cons=False):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    t0 = time.perf_counter()
    dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
    dt = time.perf_counter() - t0
    print(f"mm_mapping_align: {1e3 * dt:.1f} ms wall with the copies to the host; {int((dist >= 0).sum())} of {n} aligned, {len(ops)} runs ({4 * len(ops) / 1e6:.1f} MB)", flush=True)
    strand = rec["strand"].astype(np.int32)
    t0 = time.perf_counter()
    data, n_rec, raw = ctx.bam_encode(reads, ref, read=rec["read"], strand=strand, contig=rec["ref_contig"], dist=dist, first=first, op_off=op_off, ops=ops,
                                      flag=np.where(strand < 0, 0x10, 0), mapq=np.full(n, 60), names=[b"read%d" % r for r in rec["read"]])
    dt = time.perf_counter() - t0
    print(f"mm_bam_encode: {1e3 * dt:.1f} ms wall with the copies (the Python wrapper's own included), {n_rec} records, {raw / 1e6:.1f} MB raw, {len(data) / 1e6:.1f} MB BGZF", flush=True)
    del data
    args = dict(read=rec["read"], strand=strand, contig=rec["ref_contig"], dist=dist, first=first, op_off=op_off, ops=ops, use=np.ones(n, dtype=np.uint8))
    for rep in range(2):
        t0 = time.perf_counter()
        keys, counts = ctx.pileup_events(reads, ref, **args)
        dt = time.perf_counter() - t0
        print(f"mm_pileup_events call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(keys)} pairs of {int(counts.sum())} events ({12 * len(keys) / 1e6:.1f} MB fetched, "
              f"{12 * len(keys) / max(int((dist >= 0).sum()), 1):.0f} B per aligned read)", flush=True)
    t0 = time.perf_counter()
    mk, mc = ctx.pileup_merge(np.concatenate([keys, keys]), np.concatenate([counts, counts]))
    dt = time.perf_counter() - t0
    assert np.array_equal(mk, keys) and np.array_equal(mc, 2 * counts)
    print(f"mm_pileup_merge of the table with itself: {1e3 * dt:.1f} ms wall with the copies, {2 * len(keys)} pairs in, {len(mk)} out", flush=True)
    al = dist >= 0
    t0 = time.perf_counter()
    res = ctx.pileup_finish(ref, keys, counts, rec["ref_contig"][al], first[al], last[al])
    dt = time.perf_counter() - t0
    assert np.all(res["count"] <= res["depth"]) and int(res["alignments"].sum()) == int(al.sum()) and int(res["sum_depth"].sum()) == int((last[al] - first[al] + 1).sum())
    print(f"mm_pileup_finish (min_count 3, min_frac 0.2): {1e3 * dt:.1f} ms wall with the copies, {len(res['key'])} of {len(keys)} entries kept, "
          f"{int((res['alignments'] > 0).sum())} contigs with alignments, {int(res['covered'].sum())} positions covered, summed depth {int(res['sum_depth'].sum())}", flush=True)
    if vcf:
        del keys, counts, mk, mc, res
        for rep in range(2):
            t0 = time.perf_counter()
            w0, w1, counts = ctx.vcf_events(reads, ref, **args)
            dt = time.perf_counter() - t0
            print(f"mm_vcf_events call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(w0)} triples of {int(counts.sum())} alleles ({20 * len(w0) / 1e6:.1f} MB fetched, "
                  f"{20 * len(w0) / max(int((dist >= 0).sum()), 1):.0f} B per aligned read), {int(((w0 & 7) == 5).sum())} deletions, {int(((w0 & 7) == 6).sum())} insertions", flush=True)
        t0 = time.perf_counter()
        m0, m1, mc = ctx.vcf_merge(np.concatenate([w0, w0]), np.concatenate([w1, w1]), np.concatenate([counts, counts]))
        dt = time.perf_counter() - t0
        assert np.array_equal(m0, w0) and np.array_equal(m1, w1) and np.array_equal(mc, 2 * counts)
        print(f"mm_vcf_merge of the table with itself: {1e3 * dt:.1f} ms wall with the copies, {2 * len(w0)} triples in, {len(m0)} out", flush=True)
        del m0, m1, mc
        t0 = time.perf_counter()
        res = ctx.vcf_finish(ref, w0, w1, counts, rec["ref_contig"][al], first[al], last[al])
        dt = time.perf_counter() - t0
        print(f"mm_vcf_finish (min_count 3, min_frac 0.2): {1e3 * dt:.1f} ms wall with the copies, {len(res['w0'])} of {len(w0)} alleles kept, "
              f"{int((res['count'] > res['depth']).sum())} of them with count > depth", flush=True)
    if cons:
        clen, ic = ref.lengths(), rec["ref_contig"][al]
        groups, lo = [], 0                                          # consecutive contigs of at most 2^28 bases; a longer contig is a group alone
        while lo < len(clen):
            hi = lo + 1
            while hi < len(clen) and int(clen[lo:hi + 1].sum()) <= 1 << 28:
                hi += 1
            groups.append((lo, hi))
            lo = hi
        contigs = written = text_bytes = 0
        t0 = time.perf_counter()
        for lo, hi in groups:
            rows, ivs = ((w0 >> 35) >= lo) & ((w0 >> 35) < hi), (ic >= lo) & (ic < hi)
            got = ctx.consensus(ref, lo, hi, w0[rows], w1[rows], counts[rows], ic[ivs], first[al][ivs], last[al][ivs])
            contigs += len(got["contig"]); written += len(got["written"]); text_bytes += sum(len(t) for t in got["text"].values())
        dt = time.perf_counter() - t0
        print(f"mm_consensus (min_depth 3, min_frac 0.5, min_called 0, 60 columns): {1e3 * dt:.1f} ms wall with the copies and the Python wrapper's slicing, {len(groups)} group(s) over "
              f"{int(clen.sum())} reference bases, {contigs} contigs with alignments, {written} written, {text_bytes} bytes of text", flush=True)
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()


def child_depth(n_reads):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    dist, first, last = ctx.mapping_edit_distances(M, reads, ref, PI, n)
    al = dist >= 0
    ic, i0, i1, clen = rec["ref_contig"][al], first[al], last[al], ref.lengths()
    print(f"{int(al.sum())} intervals on {len(np.unique(ic))} of {len(clen)} contigs, {int((i1 - i0 + 1).sum())} aligned reference bases", flush=True)
    t0 = time.perf_counter()
    fin = ctx.pileup_finish(ref, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), ic, i0, i1)
    dt = time.perf_counter() - t0
    print(f"mm_pileup_finish over no entries and these intervals: {1e3 * dt:.1f} ms wall with the copies", flush=True)
    for rep, window in enumerate((1000, 1000, 1_000_000)):
        t0 = time.perf_counter()
        got = ctx.depth_profile(clen, ic, i0, i1, window=window)
        dt = time.perf_counter() - t0
        listed = got["contig"]
        assert np.array_equal(got["stats"][:, 0], fin["alignments"][listed]) and np.array_equal(got["stats"][:, 1], fin["covered"][listed]) and np.array_equal(got["stats"][:, 2], fin["sum_depth"][listed])
        assert int(got["win_sum"].sum()) == int(fin["sum_depth"].sum()) and int(got["win_covered"].sum()) == int(fin["covered"].sum())
        print(f"mm_depth_profile call {rep} (window {window}, thresholds 1,5,10,30): {1e3 * dt:.1f} ms wall with the copies and the Python wrapper, {len(got['run_contig'])} runs, "
              f"{len(listed)} contigs, {len(got['win_sum'])} windows, maximal depth {int(got['run_depth'].max())}, {int(got['stats'][:, 1].sum())} positions covered, "
              f"summed depth {int(got['stats'][:, 2].sum())}; alignments, covered and sumDepth equal mm_pileup_finish's", flush=True)
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()


def child_errprof(n_reads):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    cus = ctx.device_info()["cus"]
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings; {cus} CUs", flush=True)
    dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
    print(f"mm_mapping_align: {int((dist >= 0).sum())} of {n} aligned, {len(ops)} runs ({4 * len(ops) / 1e6:.1f} MB)", flush=True)
    args = dict(read=rec["read"], strand=rec["strand"].astype(np.int32), contig=rec["ref_contig"], dist=dist, first=first, op_off=op_off, ops=ops, use=np.ones(n, dtype=np.uint8))
    for rep in range(2):
        t0 = time.perf_counter()
        keys, counts = ctx.pileup_events(reads, ref, **args)
        dt = time.perf_counter() - t0
        print(f"mm_pileup_events call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(keys)} pairs of {int(counts.sum())} events", flush=True)
    del keys, counts
    want = None
    for per_cu in (None, None, 1, 2, 4, 8, 16, 32):                # the default twice (the first call loads the kernels), then G = per_cu * CUs
        if per_cu is None:
            os.environ.pop("MM_ERRPROF_GROUPS", None)
        else:
            os.environ["MM_ERRPROF_GROUPS"] = str(per_cu * cus)
        t0 = time.perf_counter()
        got = ctx.errprof_events(reads, ref, **args)
        dt = time.perf_counter() - t0
        want = got if want is None else want
        assert all(np.array_equal(a, b) for a, b in zip(got, want))   # no result depends on G
        print(f"mm_errprof_events call at {'the default G' if per_cu is None else f'G = {per_cu} x {cus}'}: {1e3 * dt:.1f} ms wall with the copies", flush=True)
    os.environ.pop("MM_ERRPROF_GROUPS", None)
    counters, cols, ident = want
    used = ident != np.uint64(0xFFFFFFFFFFFFFFFF)
    sub = counters[:25].reshape(5, 5)
    assert int(used.sum()) == int((dist >= 0).sum()) and int(sub.sum()) == int(cols[:, 0].sum() + cols[:, 1].sum()) and int(counters[281:281 + 95].sum()) == int(cols[:, 0].sum())
    assert int(counters[281 + 190:].sum()) == int(cols[:, 3].sum()) and int(counters[25:25 + 128].sum()) == int(cols[:, 2].sum()) and int(counters[25 + 128:281].sum()) == int(cols[:, 4].sum())
    tot = cols.sum(axis=0)
    print(f"{int(used.sum())} alignments: {int(tot[0])} matches, {int(tot[1])} mismatches, {int(tot[2])} insertions of {int(tot[3])} bases, {int(tot[4])} deletions of {int(tot[5])} bases; "
          f"{int(np.trace(sub))} columns on the diagonal; homopolymer insertions {int(counters[25 + 64:25 + 128].sum())}, deletions {int(counters[25 + 192:281].sum())}", flush=True)
    for rep in range(2):
        t0 = time.perf_counter()
        contig, stats = ctx.errprof_finish(len(ref.lengths()), ident, cols)
        dt = time.perf_counter() - t0
        assert int(stats[:-1, 0].sum()) == int(stats[-1, 0]) == int(used.sum()) and np.array_equal(stats[:-1, 1:7].sum(axis=0), stats[-1, 1:7])
        print(f"mm_errprof_finish call {rep}: {1e3 * dt:.1f} ms wall with the copies and the host's pass over the keys, {len(contig)} contigs listed; identity of all alignments "
              f"{stats[-1, 1] / max(int(stats[-1, 1] + stats[-1, 2] + stats[-1, 4] + stats[-1, 6]), 1):.6f}, per-alignment min {stats[-1, 7] / 1e6:.6f} median {stats[-1, 9] / 1e6:.6f} "
              f"max {stats[-1, 11] / 1e6:.6f}", flush=True)
    M.close(); idx.close(); reads.close(); ref.close(); ctx.close()


def child_qual(n_reads, floor):
    from metamaps_amd import capi
    ctx = capi.Context(0)
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = capi.lib().mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    synth, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    buf, ln = synth.fetch_range(0, synth.count)                     # the batch as a parser would hand it over: ASCII on the host, and seeded qualities beside it
    synth.close()
    at = np.concatenate([[0], np.cumsum(ln, dtype=np.int64)])
    text = buf.tobytes()
    seqs = [text[at[i]:at[i + 1]] for i in range(len(ln))]
    qual = np.random.default_rng(7).integers(2, 41, size=len(text), dtype=np.uint8).tobytes()
    quals = [qual[at[i]:at[i + 1]] for i in range(len(ln))]
    print(f"qualities: uniform in 2 .. 40 per base, seeded, independent of the bases and of the synthetic errors; floor {floor}", flush=True)
    sets = {}
    for rep in range(2):
        for name, q in (("without", None), ("with", quals)):
            if name in sets:
                sets[name].close()
            t0 = time.perf_counter()
            sets[name] = ctx.seqset(seqs, quals=q, qual_offset=0)
            dt = time.perf_counter() - t0
            print(f"upload {name} the quality plane, call {rep}: {1e3 * dt:.1f} ms wall (the Python wrapper's adds included), {len(text) / 4e6:.1f} MB of packed bases"
                  + (f" + {len(text) / 1e6:.1f} MB of qualities host to device" if q else ""), flush=True)
    plain, reads = sets["without"], sets["with"]
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
    strand = rec["strand"].astype(np.int32)
    jobs = dict(read=rec["read"], strand=strand, contig=rec["ref_contig"], dist=dist, first=first, op_off=op_off, ops=ops)
    bam = dict(jobs, flag=np.where(strand < 0, 0x10, 0), mapq=np.full(n, 60), names=[b"read%d" % r for r in rec["read"]])
    for rep in range(2):
        for name, S in (("without", plain), ("with", reads)):
            t0 = time.perf_counter()
            data, n_rec, raw = ctx.bam_encode(S, ref, **bam)
            dt = time.perf_counter() - t0
            print(f"mm_bam_encode {name} qualities, call {rep}: {1e3 * dt:.1f} ms wall with the copies, {n_rec} records, {raw / 1e6:.1f} MB raw, {len(data) / 1e6:.1f} MB BGZF", flush=True)
            del data
    ev = dict(jobs, use=np.ones(n, dtype=np.uint8))
    for rep in range(2):
        for q in (0, floor):
            t0 = time.perf_counter()
            keys, counts = ctx.pileup_events(reads, ref, min_base_quality=q, **ev)
            dt = time.perf_counter() - t0
            print(f"mm_pileup_events_q floor {q}, call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(keys)} pairs of {int(counts.sum())} events", flush=True)
            del keys, counts
    for rep in range(2):
        for q in (0, floor):
            t0 = time.perf_counter()
            w0, w1, counts = ctx.vcf_events(reads, ref, min_base_quality=q, **ev)
            dt = time.perf_counter() - t0
            print(f"mm_vcf_events_q floor {q}, call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(w0)} triples of {int(counts.sum())} alleles", flush=True)
            del w0, w1, counts
    M.close(); idx.close(); reads.close(); plain.close(); ref.close(); ctx.close()


MOTIFS = [("GATC", 1), ("CCWGG", 1), ("CG", 0)]                  # --motifs: Dam, Dcm and CpG


def child_mods(n_reads, motifs=False):
    import ctypes as C
    from metamaps_amd import capi
    ctx = capi.Context(0)
    L = capi.lib()
    ref = ctx.synth_reference(seed=20260928, n_species=25, strains_per_species=4, genome_len=2_200_000, strain_divergence=0.02, genus_divergence=0.2)
    w = L.mm_recommended_window(1e-3, K, PI, 1000, ref.total_bases)
    idx = ctx.index(ref, K, w)
    synth, _ = ctx.synth_reads(ref, seed=1000, n_reads=n_reads, read_len=READ_LEN, read_len_min=0, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=100)
    buf, ln = synth.fetch_range(0, synth.count)                     # the batch as a parser would hand it over: ASCII on the host, and seeded tags beside it
    synth.close()
    at = np.concatenate([[0], np.cumsum(ln, dtype=np.int64)])
    rng = np.random.default_rng(8)
    # C+m? and A+a. on EVERY C and A (all skips 0), ML bytes uniform in 0 .. 255: seeded, independent of the bases and of the synthetic errors
    base, code, mode = np.frombuffer(b"CA", dtype=np.uint8).copy(), np.array([0, 1], dtype=np.int8), np.frombuffer(b"?.", dtype=np.uint8).copy()
    n_c = np.add.reduceat((buf == 67).astype(np.int64), at[:-1]) * (ln > 0)
    n_a = np.add.reduceat((buf == 65).astype(np.int64), at[:-1]) * (ln > 0)
    calls = int(n_c.sum() + n_a.sum())
    ml = rng.integers(0, 256, size=calls, dtype=np.uint8)
    skips = np.zeros(int((n_c + n_a).max()), dtype=np.uint32)
    print(f"tags: C+m? and A+a. on every C and A, {calls} calls on {int(ln.sum())} bases, ML uniform in 0 .. 255, seeded; min_ml 204", flush=True)
    sets = {}
    for rep in range(2):
        for name in ("without", "with"):
            if name in sets:
                sets[name].close()
            t0 = time.perf_counter()
            h = C.c_void_p()
            ctx.check(L.mm_seqset_create(ctx.h, C.byref(h)))
            S = capi.SeqSet(ctx, h)
            m0 = 0
            for i in range(len(ln)):
                ctx.check(L.mm_seqset_add_view(h, buf[at[i]:].ctypes.data_as(C.c_char_p), int(ln[i])))
                if name == "with":
                    off = np.array([0, n_c[i], n_c[i] + n_a[i]], dtype=np.int64)
                    ctx.check(L.mm_seqset_add_mods(h, 2, capi._ptr(base), capi._ptr(code), capi._ptr(mode), capi._ptr(off), capi._ptr(skips), capi._ptr(ml[m0:])))
                    m0 += int(off[2])
            ctx.check(L.mm_seqset_upload(h))
            sets[name] = S
            dt = time.perf_counter() - t0
            print(f"upload {name} the modification groups, call {rep}: {1e3 * dt:.1f} ms wall (the Python wrapper's adds included), {int(ln.sum()) / 4e6:.1f} MB of packed bases"
                  + (f" + {5 * calls / 1e6:.1f} MB of skips (4 B) and ML bytes (1 B) host to device, a plane of {2 * int(ln.sum()) / 1e6:.1f} MB on the device" if name == "with" else ""), flush=True)
    plain, reads = sets["without"], sets["with"]
    M = ctx.map_batch(idx, reads, K, w, pi=PI)
    M.keep_best(K)
    off, rec = M.fetch()
    n = len(rec)
    print(f"{n_reads} reads of {READ_LEN} bases against {ref.total_bases} reference bases (k {K}, w {w}, pi {PI}): {n} best mappings", flush=True)
    dist, first, last, op_off, ops = ctx.mapping_align(M, reads, ref, PI)
    ev = dict(read=rec["read"], strand=rec["strand"].astype(np.int32), contig=rec["ref_contig"], dist=dist, first=first, op_off=op_off, ops=ops, use=np.ones(n, dtype=np.uint8))
    for rep in range(2):
        t0 = time.perf_counter()
        keys, counts = ctx.pileup_events(reads, ref, **ev)
        dt = time.perf_counter() - t0
        print(f"mm_pileup_events call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(keys)} pairs of {int(counts.sum())} events", flush=True)
        del keys, counts
        t0 = time.perf_counter()
        keys, counts = ctx.mod_events(reads, ref, **ev)
        dt = time.perf_counter() - t0
        print(f"mm_mod_events call {rep}: {1e3 * dt:.1f} ms wall with the copies, {len(keys)} pairs of {int(counts.sum())} events ({12 * len(keys) / 1e6:.1f} MB fetched), "
              f"classes {np.bincount((keys & 7).astype(np.int64), minlength=7).tolist()}", flush=True)
    assert len(ctx.mod_events(plain, ref, **ev)[0]) == 0            # (a set without a plane: the jobs are checked, nothing is counted)
    half = len(keys) // 2
    t0 = time.perf_counter()
    mk, mc = ctx.mod_merge(np.concatenate([keys[half:], keys]), np.concatenate([counts[half:], counts]))
    dt = time.perf_counter() - t0
    assert np.array_equal(mk, keys) and np.array_equal(mc[:half], counts[:half]) and np.array_equal(mc[half:], 2 * counts[half:])
    print(f"mm_mod_merge of the table with its upper half: {1e3 * dt:.1f} ms wall with the copies, {len(keys) + len(keys) - half} pairs in, {len(mk)} out", flush=True)
    del mk, mc
    t0 = time.perf_counter()
    rows = ctx.mod_finish(ref, keys, counts, "CA", 1)
    dt = time.perf_counter() - t0
    print(f"mm_mod_finish (codes C+m, A+a; min_coverage 1): {1e3 * dt:.1f} ms wall with the copies, {len(rows['site'])} rows of {len(keys)} entries, "
          f"{int(rows['n_mod'].sum())} modified, {int(rows['n_canonical'].sum())} canonical, {int(rows['n_fail'].sum())} failed calls", flush=True)
    if motifs:                                                     # the groups the CLI would make: consecutive contigs up to 2^28 bases
        lens, groups, lo, bases = ref.lengths(), [], 0, 0
        for c, n_c in enumerate(lens.tolist()):
            if c > lo and bases + n_c > (1 << 28):
                groups.append((lo, c)); lo, bases = c, 0
            bases += n_c
        groups.append((lo, len(lens)))
        for combine in (False, True):
            for rep in range(2):
                t0 = time.perf_counter()
                got = [ctx.mod_motifs(ref, a, b, keys, counts, "CA", MOTIFS, 1, 0.5, combine) for a, b in groups]
                dt = time.perf_counter() - t0
                sums = np.concatenate([g["sums"] for g in got]).sum(axis=0).tolist()
                print(f"mm_mod_motifs ({', '.join('%s:%d' % m for m in MOTIFS)}; codes C+m, A+a; min_coverage 1, min_frac 0.5, combine_strands {int(combine)}) call {rep}: {1e3 * dt:.1f} ms wall "
                      f"with the copies (every call checks the whole table on the host; only the group's slice of it goes to the device), {len(groups)} group(s) over {int(lens.sum())} reference bases, {sum(len(g['site']) for g in got)} rows, "
                      f"sums over contigs, motifs and codes: sites {sums[0]}, covered {sums[1]}, modified {sums[2]}, N_valid_cov {sums[3]}, N_mod {sums[4]}", flush=True)
    M.close(); idx.close(); reads.close(); plain.close(); ref.close(); ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--child-mods", "--child-motifs"):
        return child_mods(int(sys.argv[2]), sys.argv[1] == "--child-motifs")
    if len(sys.argv) > 1 and sys.argv[1] == "--motifs":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-motifs", str(n_reads)], env=dict(os.environ, MM_MODS_TIMING="1"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --motifs {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "motif_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--mods":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-mods", str(n_reads)], env=dict(os.environ, MM_PILEUP_TIMING="1", MM_MODS_TIMING="1"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --mods {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "mods_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-error-profile":
        return child_errprof(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--error-profile":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-error-profile", str(n_reads)], env=dict(os.environ, MM_PILEUP_TIMING="1", MM_ERRPROF_TIMING="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --error-profile {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "errprof_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-depth":
        return child_depth(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--depth":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-depth", str(n_reads)], env=dict(os.environ, MM_PILEUP_TIMING="1", MM_DEPTH_TIMING="1"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --depth {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "depth_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-qual":
        return child_qual(int(sys.argv[2]), int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == "--qualities":
        rest = sys.argv[2:]
        floor = 20
        if "--min-base-quality" in rest:
            k = rest.index("--min-base-quality")
            floor = int(rest[k + 1])
            del rest[k:k + 2]
        n_reads = int(rest[0]) if rest else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-qual", str(n_reads), str(floor)],
                           env=dict(os.environ, MM_BAM_TIMING="1", MM_PILEUP_TIMING="1", MM_VCF_TIMING="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --qualities {n_reads} --min-base-quality {floor}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "qual_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-pileup":
        return child_pileup(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-vcf":
        return child_pileup(int(sys.argv[2]), vcf=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--child-consensus":
        return child_pileup(int(sys.argv[2]), vcf=True, cons=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--consensus":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-consensus", str(n_reads)],
                           env=dict(os.environ, MM_EDIT_TIMING="1", MM_BAM_TIMING="1", MM_PILEUP_TIMING="1", MM_VCF_TIMING="1", MM_CONS_TIMING="1"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --consensus {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "consensus_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--vcf":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcf", str(n_reads)],
                           env=dict(os.environ, MM_EDIT_TIMING="1", MM_BAM_TIMING="1", MM_PILEUP_TIMING="1", MM_VCF_TIMING="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=1100)
        text = f"tools/edit_kernel_stats.py --vcf {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "vcf_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--pileup":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-pileup", str(n_reads)],
                           env=dict(os.environ, MM_EDIT_TIMING="1", MM_BAM_TIMING="1", MM_PILEUP_TIMING="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --pileup {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "pileup_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-reads-out":
        return child_reads_out(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--reads-out":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-reads-out", str(n_reads)], env=dict(os.environ, MM_READS_OUT_TIMING="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --reads-out {n_reads}: one batch of {n_reads} reads of {READ_LEN} bases, every read selected; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "reads_out_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-bam-sort":
        return child_bam_sort(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--bam-sort":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-bam-sort", str(n_reads)], env=dict(os.environ, MM_BAM_TIMING="1", MM_BAM_SORT_TIMING="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --bam-sort {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "bam_sort_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child-bam":
        return child_bam(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--bam":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-bam", str(n_reads)], env=dict(os.environ, MM_EDIT_TIMING="1", MM_BAM_TIMING="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --bam {n_reads}: one batch of {n_reads} reads, best mappings only; one run\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "bam_encode_stats.txt"), "w") as f:
            f.write(text)
        return None
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-align":
        return child_align(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--align":
        n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-align", str(n_reads)], env=dict(os.environ, MM_EDIT_TIMING="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1100)
        text = f"tools/edit_kernel_stats.py --align {n_reads}: one batch of {n_reads} reads, best mappings only; MM_EDIT_TRACE_MB {os.environ.get('MM_EDIT_TRACE_MB', 'unset')}\n" + p.stdout.decode()
        print(text)
        if p.returncode != 0:
            sys.exit(p.returncode)
        with open(os.path.join(ROOT, "profiles", "edit_trace_stats.txt"), "w") as f:
            f.write(text)
        return None
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    n_sample = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_reads), str(n_sample)], env=dict(os.environ, MM_EDIT_TIMING="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    text = f"tools/edit_kernel_stats.py {n_reads} {n_sample}: one batch of {n_reads} reads, best mappings only; host sample of {n_sample} jobs\n" + p.stdout.decode()
    print(text)
    if p.returncode != 0:
        sys.exit(p.returncode)
    with open(os.path.join(ROOT, "profiles", "edit_kernel_stats.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
