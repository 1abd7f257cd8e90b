"""What profiles/gene_kernel_stats.txt is made from: mm_gene_overlap on a problem of RefSeq shape — 10^6 mappings of 10 kb against 5 * 10^6 genes of
~1 kb on 12 000 contigs, 20 features per gene group — timed stage by stage with events on the context's stream (MM_GENE_TIMING=1, three calls in a fresh
child process), and the same join on one host thread through csrc/mm_gene_core.hpp (tools/gene_host_join.cpp, built with g++ into tools/_tmp/).
Usage: python tools/gene_kernel_stats.py [n_maps] [n_genes]      (writes profiles/gene_kernel_stats.txt)"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(n_maps, n_genes, n_contigs=12_000, feats_per_group=20, n_feats=30_000, seed=1):
    rng = np.random.default_rng(seed)
    per = n_genes // n_contigs
    off = (np.arange(n_contigs + 1, dtype=np.int64) * per)
    L = per * 1100                                                  # genes of ~1 kb tile ~90 % of a contig
    gs = np.sort(rng.integers(0, L, size=(n_contigs, per)), axis=1).ravel().astype(np.int32)
    ge = (gs + rng.integers(300, 1700, size=gs.size)).astype(np.int32)
    n_groups = gs.size * 9 // 10
    gg = rng.integers(0, n_groups, size=gs.size).astype(np.int32)
    foff = np.arange(n_groups + 1, dtype=np.int64) * feats_per_group
    feat = rng.integers(0, n_feats, size=int(foff[-1])).astype(np.int32)
    mc = rng.integers(0, n_contigs, size=n_maps).astype(np.int32)
    ms = rng.integers(0, L - 10_000, size=n_maps).astype(np.int32)
    me = (ms + 10_000).astype(np.int32)
    mi = rng.integers(8000, 10001, size=n_maps) / 100.0 / 100
    return dict(off=off, gs=gs, ge=ge, gg=gg, n_groups=n_groups, foff=foff, feat=feat, n_feats=n_feats, mc=mc, ms=ms, me=me, mi=mi)


def child(n_maps, n_genes):
    from metamaps_amd import capi
    P = problem(n_maps, n_genes)
    ctx = capi.Context(0)
    for rep in range(3):
        t0 = time.perf_counter()
        reads, median, feats, on = ctx.gene_overlap(P["off"], P["gs"], P["ge"], P["gg"], P["n_groups"], P["foff"], P["feat"], P["n_feats"], P["mc"], P["ms"], P["me"], P["mi"])
        print(f"mm_gene_overlap call {rep}: {1e3 * (time.perf_counter() - t0):.1f} ms wall with uploads, checks and copies to the host; {int(reads.sum())} pairs, "
              f"feature reads sum {int(feats.sum())}, sum of medians {float(np.nansum(median)):.6f}", flush=True)
    ctx.close()
    with tempfile.TemporaryDirectory() as d:
        for k in ("off", "gs", "ge", "gg", "foff", "feat", "mc", "ms", "me", "mi"):
            P[k].tofile(os.path.join(d, k))
        exe = os.path.join(ROOT, "tools", "_tmp", "gene_host_join")
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "gene_host_join.cpp")], check=True)
        subprocess.run([exe, d], check=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    n_maps = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_genes = int(sys.argv[2]) if len(sys.argv) > 2 else 5_000_000
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_maps), str(n_genes)], env=dict(os.environ, MM_GENE_TIMING="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    text = (f"tools/gene_kernel_stats.py {n_maps} {n_genes}: {n_maps} mappings of 10 kb against {n_genes} genes of ~1 kb on 12 000 contigs, 20 features per group\n"
            + p.stdout.decode())
    print(text)
    if p.returncode != 0:
        sys.exit(p.returncode)
    with open(os.path.join(ROOT, "profiles", "gene_kernel_stats.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
