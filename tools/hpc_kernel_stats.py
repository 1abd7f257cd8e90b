"""What profiles/hpc_kernel_stats.txt is made from: the homopolymer compression of the bench community (reference side) and of one bench-sized read
batch (10^5 reads of 10 kb) beside K1 on the same batch.  Run under `rocprofv3 --kernel-trace --stats -- python tools/hpc_kernel_stats.py [scale]`."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from metamaps_amd import capi

scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
ctx = capi.Context(0)
ng, sp, ge = max(4, int(12000 * scale)), max(2, int(3000 * scale)), max(1, int(600 * scale))
human = max(1, int(round(24 * min(scale, 1.0)))) if scale >= 0.04 else 0
ref, _ = ctx.synth_community(seed=20260928, n_genomes=ng, n_species=sp, n_genera=ge, median_len=2.0e6, sigma_len=0.6, min_len=5_000, max_len=12_000_000,
                             strain_div_min=0.001, strain_div_max=0.05, genus_div_min=0.15, genus_div_max=0.25, strain_indel_events=8,
                             human_contigs=human, human_bases=int(3.1e9 * min(scale, 1.0)), repeat_fraction=0.45, n_fraction=0.01, n_repeat_families=1000,
                             total_bases_target=int(26_762_276_280 * scale))
reads, _ = ctx.synth_reads(ref, seed=1000, n_reads=100_000, read_len=10_000, read_len_min=0, frac_random=0.05, n_abundant=100, sub_rate=0.04, ins_rate=0.03, del_rate=0.05)
for name, s, want_map in (("reference", ref, True), ("read batch", reads, False)):
    for rep in range(2):
        ctx.synchronize(); t0 = time.perf_counter()
        out = s.hpc(want_map=want_map)
        ctx.synchronize(); dt = time.perf_counter() - t0
        c, m = out if want_map else (out, None)
        print(f"{name}: {s.count} sequences, {s.total_bases} raw bases -> {c.total_bases} compressed ({c.total_bases / max(s.total_bases, 1):.4f}); mm_seqset_hpc call {dt * 1e3:.2f} ms"
              + (f"; map {m.device_bytes} bytes on the device = {m.device_bytes / max(s.total_bases, 1):.4f} per raw base" if m else ""), flush=True)
        if m:
            m.close()
        if rep == 0 or want_map:
            c.close()
for rep in range(2):                                            # K1 on the raw and on the compressed batch: its kernels appear in the same trace
    ctx.synchronize(); t0 = time.perf_counter()
    off = np.zeros(reads.count + 1, dtype=np.int64)
    ctx.check(capi.lib().mm_minimizers(ctx.h, reads.h, 16, 8, off.ctypes.data, None, None, None, 0))
    ctx.synchronize(); t1 = time.perf_counter()
    ctx.check(capi.lib().mm_minimizers(ctx.h, c.h, 16, 8, off.ctypes.data, None, None, None, 0))
    ctx.synchronize(); t2 = time.perf_counter()
    print(f"mm_minimizers call (k 16, w 8): raw batch {1e3 * (t1 - t0):.2f} ms, compressed batch {1e3 * (t2 - t1):.2f} ms", flush=True)
ctx.close()
