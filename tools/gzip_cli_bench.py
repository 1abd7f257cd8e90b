"""The CLI on the same reads as page-cached FASTQ and as a plain gzip FASTQ (one member, Python's gzip at level 6, as `gzip reads.fq` or an
archive download leaves it), the gzip through zlib's sequential reader (MM_GZIP_HOST_INFLATE=1) and on the device (mm_gzip_*): wall time,
host CPU time, the reader's phase line and identical output files; with --rocprof, the device gzip kernels' time under
`rocprofv3 --kernel-trace --stats`, and the inflated text rate of the speculative-decode kernel.

  python tools/gzip_cli_bench.py --out DIR [--batches 2] [--reads 100000] [--read-len 10000] [--cpus 16] [--rocprof]

The reads are tools/bam_cli_bench.py's FASTQ (mm_synth_reads over a synthetic reference, 'I' qualities): 1.96 Gbp at the defaults.  Every run
is pinned to --cpus CPUs (taskset) and told the same budget (MM_CPU_BUDGET).  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")

from bam_cli_bench import run_cli, same_outputs                  # noqa: E402


def make_inputs(d, batches, n_reads, read_len):
    from metamaps_amd import capi, synth
    db = synth.make_db(os.path.join(d, "db"), n_genomes=40, genome_len=1_000_000, seed=7)
    fq, fqz = os.path.join(d, "reads.fq"), os.path.join(d, "reads.fq.gz")
    ctx = capi.Context(0)
    ref = ctx.seqset([s.tobytes() for s in db.contig_seqs])
    bases = 0
    with open(fq, "wb", buffering=1 << 24) as f:
        for b in range(batches):
            rb, _t = ctx.synth_reads(ref, seed=1000 + 97 * b, n_reads=n_reads, read_len=read_len, read_len_min=0, frac_random=0.05, n_abundant=100,
                                     sub_rate=0.04, ins_rate=0.03, del_rate=0.05)
            buf, ln = rb.fetch_range(0, rb.count)
            mv, at, qual = memoryview(buf), 0, b"I" * int(ln.max())
            for r, L in enumerate(ln.tolist()):
                f.write(b"@b%dr%d\n" % (b, r)); f.write(mv[at:at + L]); f.write(b"\n+\n"); f.write(qual[:L]); f.write(b"\n")
                at += L
            bases += int(ln.sum())
            rb.close()
    ref.close(); ctx.close()
    # Python's gzip at level 6: one member, one DEFLATE stream (zlib with the gzip wrapper writes the same bytes as gzip.open would)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(fq, "rb") as f, open(fqz, "wb") as g:
        while True:
            piece = f.read(64 << 20)
            if not piece:
                break
            g.write(c.compress(piece))
        g.write(c.flush())
    return db, fq, fqz, bases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    a.cpus = max(1, min(a.cpus, len(os.sched_getaffinity(0))))
    os.makedirs(a.out, exist_ok=True)
    res = {"cpus": a.cpus}
    t0 = time.time()
    db, fq, fqz, bases = make_inputs(a.out, a.batches, a.reads, a.read_len)
    res.update(bases=bases, fastq_bytes=os.path.getsize(fq), fastq_gz_bytes=os.path.getsize(fqz), inputs_s=round(time.time() - t0, 1))
    forms = {"fastq": (fq, None), "gz_zlib": (fqz, {"MM_GZIP_HOST_INFLATE": "1"}), "gz_device": (fqz, None)}
    outs = {k: os.path.join(a.out, k, "out") for k in forms}
    for k in outs:
        os.makedirs(os.path.dirname(outs[k]), exist_ok=True)
    base = ["mapDirectly", "--all", "-r", db.fasta, "--then-classify", db.dir]
    for rep in range(a.reps):                                      # alternating: the later rounds have warm page caches for every form
        for k, (q, env) in forms.items():
            res[f"{k}_{rep}"] = run_cli([CLI] + base + ["-q", q, "-o", outs[k]], a.cpus, env)
            print(k, rep, res[f"{k}_{rep}"]["wall_s"], file=sys.stderr, flush=True)
    res["outputs_identical"] = {k: same_outputs(outs[k], outs["fastq"], [(forms[k][0], fq), (outs[k], outs["fastq"])]) for k in forms if k != "fastq"}
    if a.rocprof:
        d = os.path.join(a.out, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", CLI] + base + ["-q", fqz, "-o", outs["gz_device"] + "_prof"]
        # (MM_CLI_FULL_TEARDOWN: the CLI leaves through exit() instead of _exit(), so the profiler's exit handlers write their files)
        subprocess.run(cmd, capture_output=True, text=True, timeout=1800, check=True, env=dict(os.environ, MM_CPU_BUDGET=str(a.cpus), MM_CLI_FULL_TEARDOWN="1"))
        kern = {}
        for fcsv in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fcsv)):
                if "gz_" in row["Name"]:
                    name = re.search(r"(gz_\w+)", row["Name"]).group(1)
                    kern[name] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
        res["kernels"] = kern
        spec_ms = kern.get("gz_jobs_kernel", {}).get("total_ms", 0)
        res["jobs_kernel_GBps_of_text"] = round(res["fastq_bytes"] / 1e9 / (spec_ms / 1e3), 2) if spec_ms else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
