"""What profiles/lca_kernel_stats.txt is made from: mm_em_run, mm_em_posteriors and mm_em_lca on an EM problem of bench size (10^6 reads, ~4.2
mappings per read, tools/em_latency.py's problem()) over a taxonomy-shaped tree, under one `rocprofv3 --kernel-trace --stats` run that this
script starts for itself (a fresh child process; the program goes behind `--`).  Prints the rows of the em_* and lca_* kernels of that trace:
the em_* rows are what the same entries cost before the assignment existed.
Usage: python tools/lca_kernel_stats.py [n_reads] [threshold]"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def tree_over(n_taxa, rng):
    """a taxonomy-shaped tree over n_taxa strains: root - 3 superkingdoms - 40 phyla - 400 families - n/12 genera - n/4 species - strains;
    parents before children.  Returns (parent, taxon_node)."""
    levels = [1, 3, 40, 400, max(1, n_taxa // 12), max(1, n_taxa // 4), n_taxa]
    parent, first = [0], [0]
    for lv in range(1, len(levels)):
        first.append(len(parent))
        up = np.sort(rng.integers(0, levels[lv - 1], size=levels[lv]))
        parent.extend((first[lv - 1] + up).tolist())
    return np.array(parent, dtype=np.int32), (first[-1] + np.arange(n_taxa)).astype(np.int32)


def child(n_reads, tau):
    from em_latency import problem
    from metamaps_amd import capi
    off, taxon, mapq, inv, T = problem(n_reads)
    parent, taxon_node = tree_over(T, np.random.default_rng(2))
    ctx = capi.Context(0)
    em = ctx.em(off, taxon, mapq, inv, T)
    f, lls = em.run(np.full(T, 1.0 / T))
    for rep in range(3):
        ctx.synchronize(); t0 = time.perf_counter()
        em.posteriors(f)
        ctx.synchronize(); t1 = time.perf_counter()
        node, mass, direct = em.lca(f, parent, taxon_node, tau)
        ctx.synchronize(); t2 = time.perf_counter()
        print(f"{n_reads} reads, {len(taxon)} mappings, tree of {len(parent)} nodes, tau {tau}: mm_em_posteriors call {1e3 * (t1 - t0):.2f} ms, "
              f"mm_em_lca call {1e3 * (t2 - t1):.2f} ms (both with their copies to the host); {len(lls)} EM iterations; "
              f"{int((node == taxon_node[taxon[off[:-1]]]).sum())} reads stay on their first taxon, {int((direct > 0).sum())} nodes used", flush=True)
    em.close(); ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), float(sys.argv[3]))
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    tau = float(sys.argv[2]) if len(sys.argv) > 2 else 0.8
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--",
                            sys.executable, os.path.abspath(__file__), "--child", str(n_reads), str(tau)], timeout=1500)
        if p.returncode != 0:
            sys.exit(p.returncode)
        rows = []
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(fn)))
    print(f"{'kernel':<60} {'calls':>7} {'total us':>12} {'mean us':>10} {'%':>6}")
    for r in rows:
        name = r.get("Name", "")
        if "em_" in name or "lca_" in name or "boot_" in name:
            print(f"{name[:60]:<60} {r.get('Calls', ''):>7} {float(r.get('TotalDurationNs', 0)) / 1e3:12.1f} {float(r.get('AverageNs', 0)) / 1e3:10.1f} {r.get('Percentage', ''):>6}")


if __name__ == "__main__":
    main()
