"""The CLI's mapping phase with the mappings written plain, with --compress-output deflated on the device (mm_bgzf_deflate) and with
--compress-output deflated by zlib level 1 on the host (MM_DEFLATE_HOST=1), in alternation: wall time, the phase laps, the size of PREFIX /
PREFIX.gz, the ratio against zlib level 1 on the same 65 280-byte blocks, then `classify` from each; with --rocprof, the deflate kernel's
time under `rocprofv3 --kernel-trace --stats` and its rate in GB/s of text.

  python tools/deflate_cli_bench.py --out DIR [--batches 10] [--reads 100000] [--read-len 10000] [--cpus 16] [--reps 3] [--rocprof]

The reads are tools/gzip_cli_bench.py's FASTQ (mm_synth_reads over a synthetic reference of 40 genomes of 1 Mbp); --batches 10 gives the
10^6 reads of the bench.  Every run is pinned to --cpus CPUs (taskset) and told the same budget (MM_CPU_BUDGET).  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import glob
import gzip
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")

from bam_cli_bench import run_cli                                # noqa: E402
from gzip_cli_bench import make_inputs                           # noqa: E402

EM = (".EM", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.WIMP", ".EM.lengthAndIdentitiesPerMappingUnit", ".EM.contigCoverage", ".EM.evidenceUnknownSpecies")


def zlib1_size(path):
    total = 0
    with open(path, "rb") as f:
        while True:
            b = f.read(0xff00)
            if not b:
                return total
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            total += len(c.compress(b) + c.flush()) + 26


def same_file(a, b):
    return os.path.exists(a) == os.path.exists(b) and (not os.path.exists(a) or open(a, "rb").read() == open(b, "rb").read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    a.cpus = max(1, min(a.cpus, len(os.sched_getaffinity(0))))
    os.makedirs(a.out, exist_ok=True)
    res = {"cpus": a.cpus, "reads": a.batches * a.reads}
    db, fq, _fqz, bases = make_inputs(a.out, a.batches, a.reads, a.read_len)
    res["bases"] = bases
    forms = {"plain": ([], None), "device": (["--compress-output"], None), "host_zlib1": (["--compress-output"], {"MM_DEFLATE_HOST": "1"})}
    outs = {k: os.path.join(a.out, k, "out") for k in forms}
    for k in outs:
        os.makedirs(os.path.dirname(outs[k]), exist_ok=True)
    base = ["mapDirectly", "--all", "-r", db.fasta, "-q", fq]
    for rep in range(a.reps):                                      # alternating on one box
        for k, (flags, env) in forms.items():
            r = run_cli([CLI] + base + flags + ["-o", outs[k]], a.cpus, env)
            r["mapping_phase_s"] = round(r["wall_s"] - r["laps"].get("3 index build", 0.0), 3)   # behind context, reference and index build
            res[f"map_{k}_{rep}"] = r
            print(k, rep, r["wall_s"], r["mapping_phase_s"], file=sys.stderr, flush=True)
    text = os.path.getsize(outs["plain"])
    res.update(mappings_bytes=text, lines=sum(1 for _ in open(outs["plain"], "rb")), zlib1_blocks_bytes=zlib1_size(outs["plain"]))
    for k in ("device", "host_zlib1"):
        z = os.path.getsize(outs[k] + ".gz")
        res[f"{k}_gz_bytes"] = z
        res[f"{k}_ratio"] = round(text / z, 3)
        res[f"{k}_over_zlib1"] = round(z / res["zlib1_blocks_bytes"], 4)
        with gzip.open(outs[k] + ".gz", "rb") as g, open(outs["plain"], "rb") as p:
            same = True
            while same:
                x, y = g.read(1 << 24), p.read(1 << 24)
                same = x == y
                if not x and not y:
                    break
        res[f"{k}_gunzips_to_plain"] = same
    for rep in range(a.reps):
        for k in forms:
            r = run_cli([CLI, "classify", "--DB", db.dir, "--mappings", outs[k]], a.cpus, None)
            res[f"classify_{k}_{rep}"] = {"wall_s": r["wall_s"], "cpu_user_s": r["cpu_user_s"]}
    res["classify_outputs_identical"] = {k: all(same_file(outs[k] + s, outs["plain"] + s) for s in EM) for k in ("device", "host_zlib1")}
    if a.rocprof:
        d = os.path.join(a.out, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", CLI] + base + ["--compress-output", "-o", outs["device"] + "_prof"]
        # (full teardown: the CLI leaves through exit() instead of _exit(), so the profiler's exit handlers write their files)
        subprocess.run(cmd, capture_output=True, text=True, timeout=1800, check=True, env=dict(os.environ, MM_CPU_BUDGET=str(a.cpus), MM_CLI_FULL_TEARDOWN="1"))
        for fcsv in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fcsv)):
                if "bgzf_deflate_kernel" in row["Name"]:
                    ms = float(row["TotalDurationNs"]) / 1e6
                    res["deflate_kernel"] = {"calls": int(row["Calls"]), "total_ms": round(ms, 3), "percent_of_kernel_time": float(row["Percentage"]),
                                             "GBps_of_text": round(text / 1e9 / (ms / 1e3), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
