"""The cases of tests/test_gpu_boot_edges.py (tests/boot_cases.py) are what the GPU tests take them for, from the exact reference alone: no
device, no library.  Also the weighted reference against its own unit-weight form."""
import numpy as np

import boot_cases as bc
import post_ref
from test_gpu_post_edges import LOOP_PROBLEMS, TAXON_ENTRIES, default_grid


def test_unit_weights_leave_the_reference_unchanged():
    for name in ("mappings_per_read", "fewer_reads_than_rows_17", "slow"):
        off, taxon, mapq, inv, T = bc.problem(name)
        plain = post_ref.em_reference(off, taxon, mapq, inv, T, bc.f_start(name))
        ones = post_ref.em_reference(off, taxon, mapq, inv, T, bc.f_start(name), w=np.ones(len(off) - 1, dtype=np.int64))
        assert np.array_equal(plain[0], ones[0]) and np.array_equal(plain[1], ones[1]) and plain[2] == ones[2]
        capped = post_ref.em_reference(off, taxon, mapq, inv, T, bc.f_start(name), max_iter=2)
        assert np.array_equal(capped[1], plain[1][:2])


def test_a_weight_of_two_is_the_read_twice_and_zero_is_the_read_left_out():
    off, taxon, mapq, inv, T = bc.problem("fewer_reads_than_rows_3")
    n = len(off) - 1
    w = post_ref.boot_weights(off, bc.SEED, 0)
    assert set(w.tolist()) >= {0, 1, 2}
    idx = [np.arange(off[r], off[r + 1]) for r in range(n) for _ in range(int(w[r]))]
    sel = np.concatenate(idx)
    off2 = np.concatenate([[0], np.cumsum([len(x) for x in idx])]).astype(np.int64)
    f_w, ll_w, _ = post_ref.em_reference(off, taxon, mapq, inv, T, bc.f_start("fewer_reads_than_rows_3"), w=w)
    f_d, ll_d, _ = post_ref.em_reference(off2, taxon[sel], mapq[sel], inv[sel], T, bc.f_start("fewer_reads_than_rows_3"))
    assert len(ll_w) == len(ll_d) and np.allclose(ll_w, ll_d, rtol=1e-14, atol=0) and np.allclose(f_w, f_d, rtol=1e-13, atol=0)


def test_weights_sit_at_the_index_among_the_mapped_reads():
    from test_boot_core import weights_np
    off = bc.problem("three_reads")[0]
    assert np.diff(off).tolist() == [0, 2, 0, 3, 0, 2, 0]
    g = weights_np(np.uint64(bc.SEED), np.uint64(3), np.arange(3, dtype=np.uint64))
    assert post_ref.boot_weights(off, bc.SEED, 3).tolist() == [0, g[0], 0, g[1], 0, g[2], 0]
    assert post_ref.boot_weights(off, row=[5, 0, 255]).tolist() == [0, 5, 0, 0, 0, 255, 0]
    assert np.array_equal(bc.generated_matrix("three_reads", 3, 1)[0], g)
    for name in LOOP_PROBLEMS:                                      # a kernel that took the weight at the read's own index would be seen
        sizes = np.diff(bc.problem(name)[0])
        mapped = sizes > 0
        mread = np.cumsum(mapped) - 1
        moved = np.count_nonzero(mapped & (mread != np.arange(len(sizes))))
        assert 3 * moved >= np.count_nonzero(mapped), (name, moved)
        by_own_index = weights_np(np.uint64(bc.SEED), np.uint64(0), np.arange(len(sizes), dtype=np.uint64))
        assert np.count_nonzero(by_own_index[mapped] != post_ref.boot_weights(bc.problem(name)[0], bc.SEED, 0)[mapped]) > 0.2 * moved


def test_the_shapes_the_kernels_were_written_around_are_there():
    sizes = set(np.diff(bc.problem("mappings_per_read")[0]).tolist())
    assert {7, 8, 9, 16, 17} <= sizes
    off, taxon, _, _, T = bc.problem("entries_per_taxon")
    assert {511, 512, 513, 4_097} <= set(np.bincount(taxon, minlength=T).tolist()) and set(TAXON_ENTRIES) >= {511, 512, 513, 4_097}
    for n in bc.ROWS_PRESENT:
        off, taxon, _, _, T = bc.problem(f"fewer_reads_than_rows_{n}")
        assert len(np.unique(taxon)) == n and len(off) - 1 == 40 < 256 and np.count_nonzero(np.diff(off) == 0) >= 2
    for n in bc.ROWS_WORKGROUPS:
        off, taxon, _, _, T = bc.problem(f"workgroups_{n}")
        assert len(off) - 1 == n and default_grid(n, len(taxon)) == (n, 1)
    off, taxon, _, _, T = bc.problem("three_reads")
    assert T == 5 and sorted(np.unique(taxon).tolist()) == [1, 3] and bc.mapped_reads("three_reads") == 3
    assert bc.mapped_reads("one_read") == 1 and bc.mapped_reads("no_mapping") == 0 and len(bc.problem("no_mapping")[0]) - 1 == 5


def test_empty_replicates():
    assert bc.empty_replicates("three_reads", 129) == [7, 18, 54, 69, 86, 126]
    assert len(bc.empty_replicates("one_read", 256)) == 95
    for r in range(bc.EMPTY_B):
        f, ll, n_iter, stopped, _ = bc.expected(bc.EMPTY, r)
        if r in (7, 18, 54, 69, 86, 126):
            assert not f.any() and ll == 0 and n_iter == 0 and stopped
        else:
            assert n_iter > 0 and abs(f.sum() - 1) < 1e-12 and ll < 0
    assert bc.expected("one_read", 1)[2] == 0 and bc.expected("one_read", 63)[2] == 0 and bc.expected("one_read", 2)[2] > 0
    assert [bc.expected(bc.EMPTY, None, "zero_row", k)[2] > 0 for k in range(3)] == [True, False, True]
    off, taxon, mapq, inv, T = bc.problem("no_mapping")
    assert post_ref.boot_expected(off, taxon, mapq, inv, T, bc.f_start("no_mapping"), post_ref.boot_weights(off, bc.SEED, 0))[1:4] == (0.0, 0, True)


def test_replicates_of_one_tile_stop_in_different_iterations():
    it = bc.iterations(bc.TILE, range(65))
    assert len(set(it)) >= 3, sorted(set(it))
    assert any(it[r] < it[r + 1] for r in range(63)) and any(it[r] < it[r - 1] for r in range(1, 64))   # earlier than the next lane, than the previous
    assert it[63] != it[64] or it[0] != it[64]
    reps = bc.tile_reps()
    all_it = bc.iterations(bc.TILE, range(129))
    assert {0, 63, 64} <= set(reps) and min(all_it) in [all_it[r] for r in reps] and max(all_it) in [all_it[r] for r in reps]


def test_caps_cut_some_replicates_and_not_others():
    full = bc.iterations("slow", range(bc.CAP_B))
    assert min(full) < 23 and any(25 < n <= 32 for n in full) and max(full) > 33, full
    for cap in bc.CAPS:
        for r in range(bc.CAP_B):
            _, _, n_iter, stopped, _ = bc.expected("slow", r, None, None, cap)
            assert n_iter == min(full[r], cap) and stopped == (full[r] <= cap)


def test_stop_margins_of_every_compared_pair():
    """the device may differ from the reference in the last bits of a log-likelihood: no compared replicate may decide its stop on them"""
    worst = 1.0
    pairs = bc.compared()
    assert len(pairs) == len(set(pairs)) > 200
    for c in pairs:
        margins = bc.expected(*c)[4]
        for gain_off, rel_off in margins[-2:]:
            assert gain_off >= 1e-6 and rel_off >= 1e-6, (c, margins[-2:])
            worst = min(worst, gain_off, rel_off)
    print(f"smallest stop margin of the last two iterations over {len(pairs)} pairs: {worst:.3g}")
