"""What profiles/ident_filter_stats.txt is made from: mm_ident_filter on an EM problem of bench size (10^6 reads, ~4.2 mappings per read over 300 of
12 001 taxa, tools/em_latency.py's problem(); every taxon with its own level of identity) timed stage by stage with events on the context's stream
(MM_IDENT_TIMING=1, three calls in a fresh child process), and the same filter on one host thread through csrc/mm_ident_core.hpp
(tools/ident_host_filter.cpp, built with g++ into tools/_tmp/).
Usage: python tools/ident_filter_stats.py [n_reads] [threshold in percent]      (writes profiles/ident_filter_stats.txt)"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(n_reads, thr):
    from em_latency import problem
    from metamaps_amd import capi
    off, taxon, _, _, T = problem(n_reads)
    rng = np.random.default_rng(3)
    level = rng.uniform(75, 97, size=T)
    ident = np.round(np.clip(level[taxon] + rng.normal(0, 3, size=len(taxon)), 0, 100), 4)
    best = off[:-1].copy()                                          # (the read's true taxon)
    ctx = capi.Context(0)
    for rep in range(3):
        t0 = time.perf_counter()
        r = ctx.ident_filter(off, taxon, ident, best, T, thr)
        print(f"mm_ident_filter call {rep}: {1e3 * (time.perf_counter() - t0):.1f} ms wall with uploads, checks and copies to the host; "
              f"{int(r['taxon_removed'].sum())} of the genomes removed, {len(r['read_src'])} reads and {len(r['entry_src'])} entries kept, n_le {r['n_le']}", flush=True)
    ctx.close()
    with tempfile.TemporaryDirectory() as d:
        for k, a in (("off", off), ("taxon", taxon.astype(np.int32)), ("ident", ident), ("best", best.astype(np.int64))):
            a.tofile(os.path.join(d, k))
        exe = os.path.join(ROOT, "tools", "_tmp", "ident_host_filter")
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "ident_host_filter.cpp")], check=True)
        subprocess.run([exe, d, str(T), repr(thr)], check=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), float(sys.argv[3]))
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    thr = float(sys.argv[2]) if len(sys.argv) > 2 else 85.0
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_reads), str(thr)], env=dict(os.environ, MM_IDENT_TIMING="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    text = f"tools/ident_filter_stats.py {n_reads} {thr}: {n_reads} reads of the bench's EM shape, threshold {thr} %\n" + p.stdout.decode()
    print(text)
    if p.returncode != 0:
        sys.exit(p.returncode)
    with open(os.path.join(ROOT, "profiles", "ident_filter_stats.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
