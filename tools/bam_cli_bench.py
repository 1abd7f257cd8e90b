"""The CLI on the same reads as page-cached FASTQ, as unaligned BAM and as bgzip-compressed FASTQ, the BGZF forms each with device inflate
(mm_bgzf_inflate) and with host inflate (MM_BGZF_HOST_INFLATE=1: zlib on a TaskPool for BAM, zlib's sequential gzread for bgzip text): wall
time, host CPU time and identical output files, the BAM reader's host inflate rate (tests/test_bam_reader.cpp, `rate` mode) and, with
--rocprof, the device pack and inflate kernels' time under `rocprofv3 --kernel-trace --stats` (one run per BGZF form).

  python tools/bam_cli_bench.py --out DIR [--batches 2] [--reads 100000] [--read-len 10000] [--cpus 16] [--rocprof]

Reads come from the device's read synthesiser (mm_synth_reads, the generator of bench.py's batches) over a synthetic reference; the BAM stores
every other read reverse-complemented (0x10) and qualities drawn from a fixed distribution of Phred 5-40, as a basecaller writes them (the
FASTQ carries 'I': the mapper reads no qualities).  Every run is pinned to --cpus CPUs (taskset) and told the same budget (MM_CPU_BUDGET).
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import re
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")

_LUT = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _LUT[_c] = _i
_COMP = np.array([int(f"{i:04b}"[::-1], 2) for i in range(16)], dtype=np.uint8)


def _deflate(chunk: bytes) -> bytes:
    import bam_writer as bw
    return bw.bgzf_block(chunk, level=1)


def _deflate6(chunk: bytes) -> bytes:                             # (bgzip's default level)
    import bam_writer as bw
    return bw.bgzf_block(chunk, level=6)


def _records(buf, ln, names, rng):
    import struct
    out, at = [], 0
    for r, L in enumerate(ln.tolist()):
        codes = _LUT[buf[at:at + L]]
        at += L
        flag = 0x10 if r % 2 else 0
        if flag:
            codes = _COMP[codes[::-1]]
        if L % 2:
            codes = np.append(codes, 0)
        packed = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes()
        qual = rng.integers(5, 41, L, dtype=np.uint8).tobytes()
        nm = names[r] + b"\0"
        body = struct.pack("<iiBBHHHi", -1, -1, len(nm), 255, 4680, 0, flag, L) + struct.pack("<iii", -1, -1, 0) + nm + packed + qual
        out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


def make_inputs(d, batches, n_reads, read_len, cpus):
    from metamaps_amd import capi, synth
    import bam_writer as bw
    db = synth.make_db(os.path.join(d, "db"), n_genomes=40, genome_len=1_000_000, seed=7)
    fq, bam, fqz = os.path.join(d, "reads.fq"), os.path.join(d, "reads.bam"), os.path.join(d, "reads.fq.gz")
    ctx = capi.Context(0)
    ref = ctx.seqset([s.tobytes() for s in db.contig_seqs])
    rng = np.random.default_rng(5)
    bases = 0
    with open(fq, "wb", buffering=1 << 24) as f, open(bam, "wb") as g, mp.Pool(cpus) as pool:
        pend = bw.header_bytes(refs=())
        bam_inflated = len(pend)
        for b in range(batches):
            rb, _t = ctx.synth_reads(ref, seed=1000 + 97 * b, n_reads=n_reads, read_len=read_len, read_len_min=0, frac_random=0.05, n_abundant=100,
                                     sub_rate=0.04, ins_rate=0.03, del_rate=0.05)
            buf, ln = rb.fetch_range(0, rb.count)
            names = [b"b%dr%d" % (b, r) for r in range(len(ln))]
            mv, at, qual = memoryview(buf), 0, b"I" * int(ln.max())
            for r, L in enumerate(ln.tolist()):
                f.write(b"@" + names[r] + b"\n"); f.write(mv[at:at + L]); f.write(b"\n+\n"); f.write(qual[:L]); f.write(b"\n")
                at += L
            bases += int(ln.sum())
            recs = _records(buf, ln, names, rng)
            bam_inflated += len(recs)
            pend += recs
            cut = len(pend) // 65280 * 65280
            for blk in pool.imap(_deflate, [pend[i:i + 65280] for i in range(0, cut, 65280)], chunksize=64):
                g.write(blk)
            pend = pend[cut:]
            rb.close()
        for blk in pool.imap(_deflate, [pend[i:i + 65280] for i in range(0, len(pend), 65280)]):
            g.write(blk)
        g.write(bw.EOF_BLOCK)
    ref.close(); ctx.close()
    with open(fq, "rb") as f, open(fqz, "wb") as g, mp.Pool(cpus) as pool:   # what `bgzip reads.fq` writes
        while True:
            piece = f.read(65280 * 1024)
            if not piece:
                break
            for blk in pool.imap(_deflate6, [piece[i:i + 65280] for i in range(0, len(piece), 65280)], chunksize=16):
                g.write(blk)
        g.write(bw.EOF_BLOCK)
    return db, fq, bam, fqz, bases, bam_inflated


def run_cli(cmd, cpus, env_extra=None):
    env = dict(os.environ, MM_CLI_TIMING="1", MM_CPU_BUDGET=str(cpus), **(env_extra or {}))
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.time()
    p = subprocess.run(["taskset", "-c", f"0-{cpus - 1}"] + cmd, capture_output=True, text=True, env=env, timeout=1800)
    wall = time.time() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if p.returncode != 0:
        raise SystemExit(f"{cmd[:3]} failed ({p.returncode}): {p.stderr[-2000:]}")
    laps = {ln.split(" at +")[0][len("INFO, lap "):]: float(ln.split(" at +")[1].split()[0]) for ln in p.stderr.splitlines() if ln.startswith("INFO, lap ")}
    times = {" ".join(ln.split()[2:-2]): float(ln.split()[-2]) for ln in p.stderr.splitlines() if ln.startswith("INFO, time ")}
    return {"wall_s": round(wall, 3), "cpu_user_s": round(r1.ru_utime - r0.ru_utime, 2), "cpu_sys_s": round(r1.ru_stime - r0.ru_stime, 2),
            "laps": laps, "reader": {k: v for k, v in times.items() if k.startswith("R ")}}


def same_outputs(a, b, subst):
    sufs = ("", ".meta", ".meta.unmappedReadsLengths", ".parameters", ".EM", ".EM.reads2Taxon", ".EM.WIMP", ".EM.contigCoverage")
    for s in sufs:
        x, y = open(a + s, "rb").read(), open(b + s, "rb").read()
        for u, v in subst:
            x = x.replace(u.encode(), v.encode())
        if x != y:
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--prof-dir", default=None, help="where rocprofv3 writes (default: under --out)")
    a = ap.parse_args()
    a.cpus = max(1, min(a.cpus, len(os.sched_getaffinity(0))))
    os.makedirs(a.out, exist_ok=True)
    res = {"cpus": a.cpus}
    t0 = time.time()
    db, fq, bam, fqz, bases, bam_inflated = make_inputs(a.out, a.batches, a.reads, a.read_len, a.cpus)
    res.update(bases=bases, fastq_bytes=os.path.getsize(fq), bam_bytes=os.path.getsize(bam), bam_inflated_bytes=bam_inflated,
               fastq_gz_bytes=os.path.getsize(fqz), inputs_s=round(time.time() - t0, 1))
    rate_exe = os.path.join(a.out, "bam_rate")
    subprocess.run(["g++", "-O3", "-std=c++17", "-pthread", "-o", rate_exe, os.path.join(ROOT, "tests", "test_bam_reader.cpp"), "-lz"], check=True)
    for t in sorted({1, max(1, a.cpus // 2), a.cpus}):
        p = subprocess.run(["taskset", "-c", f"0-{a.cpus - 1}", rate_exe, "rate", bam, str(t)], capture_output=True, text=True, timeout=900, check=True)
        res[f"reader_rate_threads{t}"] = p.stdout.strip()
    host = {"MM_BGZF_HOST_INFLATE": "1"}
    dev = {"MM_BAM_DEVICE_INFLATE": "1"}
    forms = {"fastq": (fq, None), "bam_device": (bam, dev), "bam_host": (bam, host), "fqgz_device": (fqz, None), "fqgz_host": (fqz, host)}
    outs = {k: os.path.join(a.out, k, "out") for k in forms}
    for k in outs:
        os.makedirs(os.path.dirname(outs[k]), exist_ok=True)
    base = ["mapDirectly", "--all", "-r", db.fasta, "--then-classify", db.dir]
    for rep in range(2):                                           # alternating, twice: the second round has warm page caches for every form
        for k, (q, env) in forms.items():
            res[f"{k}_{rep}"] = run_cli([CLI] + base + ["-q", q, "-o", outs[k]], a.cpus, env)
    res["outputs_identical"] = {k: same_outputs(outs[k], outs["fastq"], [(forms[k][0], fq), (outs[k], outs["fastq"])]) for k in forms if k != "fastq"}
    if a.rocprof:
        import csv
        import glob
        res["kernels"] = {}
        for k, q, inflated in (("bam_device", bam, bam_inflated), ("fqgz_device", fqz, res["fastq_bytes"])):
            d = os.path.join(a.prof_dir or os.path.join(a.out, "prof"), k)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", CLI] + base + ["-q", q, "-o", outs[k] + "_prof"]
            # (MM_CLI_FULL_TEARDOWN: the CLI leaves through exit() instead of _exit(), so the profiler's exit handlers write their files)
            subprocess.run(cmd, capture_output=True, text=True, timeout=1800, check=True, env=dict(os.environ, MM_CPU_BUDGET=str(a.cpus), MM_CLI_FULL_TEARDOWN="1", **dev))
            kern = {}
            for fcsv in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(fcsv)):
                    if "nt16" in row["Name"] or "scan_" in row["Name"] or "bgzf" in row["Name"]:
                        name = re.search(r"(\w+)(<[^(]*>)?\(", row["Name"]).group(1)   # (names carry namespaces, "(anonymous namespace)" among them)
                        kern[name] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
            res["kernels"][k] = kern
            inf_ms = sum(v["total_ms"] for n, v in kern.items() if "bgzf" in n)
            res[f"{k}_inflate_kernel_GBps"] = round(inflated / 1e9 / (inf_ms / 1e3), 2) if inf_ms else None
            res[f"{k}_inflate_kernel_ms"] = round(inf_ms, 2)
            if k == "bam_device":
                nt16_ms = sum(v["total_ms"] for n, v in kern.items() if "nt16" in n)
                res["nt16_kernels_ms_per_gbase"] = round(nt16_ms / (bases / 1e9), 3) if bases else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
