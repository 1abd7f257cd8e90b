"""Wall time of the EM bootstrap (mm_em_bootstrap) on a problem of the bench's shape (tools/em_latency.py's problem()): B replicates in one
batched call against single-replicate calls one after the other, the iterations per replicate, and the bytes the phases move per iteration
computed from the shapes (to set against `rocprofv3 --kernel-trace --stats` times of boot_p1/p2/p3_kernel).  Prints one line per measurement.
Usage: python tools/em_bootstrap_time.py [n_reads] [B] [n_sequential]   (the sequential time is scaled from n_sequential calls to B)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from metamaps_amd import capi
from em_latency import problem


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    n_seq = int(sys.argv[3]) if len(sys.argv) > 3 else B
    off, taxon, mapq, inv, T = problem(n_reads)
    ne = len(taxon)
    ctx = capi.Context(0)
    e = ctx.em(off, taxon, mapq, inv, T)
    f_hat, lls = e.run(np.full(T, 1.0 / T), max_iter=10_000)
    print(f"{n_reads} reads, {ne} mappings, {T} taxa ({np.count_nonzero(np.bincount(taxon, minlength=T))} present); point EM {len(lls)} iterations")
    e.bootstrap(f_hat, 2, seed=1, max_iter=3)                     # first launches, the loop's set-up
    ctx.synchronize()
    t0 = time.perf_counter()
    f, ll, it, st = e.bootstrap(f_hat, B, seed=1)
    t_batch = time.perf_counter() - t0
    print(f"batched: B={B} in {t_batch * 1e3:.1f} ms; iterations per replicate min {it.min()} median {int(np.median(it))} max {it.max()} "
          f"(the loop runs {it.max()}); stop rule met by {int(st.sum())}")
    t0 = time.perf_counter()
    it_seq = []
    for r in range(n_seq):
        _, _, i1, _ = e.bootstrap(f_hat, 1, seed=1, rep0=r)
        it_seq.append(int(i1[0]))
    t_seq = (time.perf_counter() - t0) * B / n_seq
    print(f"sequential: {n_seq} single-replicate calls, {t_seq * 1e3:.1f} ms scaled to {B}, {sum(it_seq) / n_seq:.1f} iterations per call; "
          f"batched speed-up {t_seq / t_batch:.1f}x")
    tiles = -(-B // 64)
    p1 = ne * B * 8 + ne * 28 * tiles                             # posteriors written; taxon / inv_nloc / mapq / pos read once per tile (f gathers: cache)
    p2 = ne * B * 8                                               # posteriors read
    print(f"bytes per iteration: P1b {p1 / 1e6:.1f} MB, P2b {p2 / 1e6:.1f} MB; at 6.3 TB/s {(p1 + p2) / 6.3e12 * 1e6:.1f} us")
    e.close(); ctx.close()


if __name__ == "__main__":
    main()
