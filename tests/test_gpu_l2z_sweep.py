"""The zone kernel's sweep (mm_l2z.hpp) against l2_kernel, one wave per candidate (MM_L2_V1=1), and its hand-back of candidates to l2_kernel.

The block search between sweeps picks the next block whose bound passes by two ballots over the bounds (10 kb class); MM_L2Z_WALK_SEARCH makes it
walk the blocks one at a time as the long-read classes do, and the two must visit the same blocks.  The pass-count guard of the band loop
hands an unfinished candidate to l2_kernel through the big list.  MM_L2Z_FORCE_HANDBACK sends every candidate that reaches the band loop that way,
so the hand-back path must give the records the default path gives.  Reads of 1-30 kb on a repeat-rich reference (duplicate hashes: DP/DN flags)
take both the 10 kb and the long-read classes."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_zone_sweep_and_handback_equal_rank_code_kernel(ctx, monkeypatch):
    ref, _genome = ctx.synth_community(seed=29, n_genomes=24, n_species=8, n_genera=3, median_len=200_000.0, sigma_len=0.5, min_len=20_000, max_len=500_000,
                                       strain_div_min=0.001, strain_div_max=0.05, genus_div_min=0.15, genus_div_max=0.25, strain_indel_events=6,
                                       human_contigs=2, human_bases=3_000_000, repeat_fraction=0.45, n_fraction=0.01, n_repeat_families=12, total_bases_target=0)
    reads, _ = ctx.synth_reads(ref, seed=43, n_reads=3000, read_len=30_000, read_len_min=1_000, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=31)
    idx = ctx.index(ref, 16, 8)
    res = {}
    for mode, env in (("zone", {}), ("walk", {"MM_L2Z_WALK_SEARCH": "1"}), ("handback", {"MM_L2Z_FORCE_HANDBACK": "1"}), ("zone_two_pass", {"MM_L2_NO_FUSE": "1"}),
                      ("rank_codes", {"MM_L2_V1": "1"})):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        M = ctx.map_batch(idx, reads, 16, 8)
        off, rec = M.fetch()
        st = M.stats()
        res[mode] = (off.copy(), rec.copy(), M.debug_l2(st["n_candidates"]), st)
        M.close()
        for k_ in env:
            monkeypatch.delenv(k_)
    base = res["rank_codes"]
    assert base[3]["n_candidates"] > 5_000 and base[3]["n_mappings"] > 2_000
    # every candidate the zone kernel reached its band loop with went to l2_kernel
    assert res["handback"][3]["n_l2_wide_redo"] > res["zone"][3]["n_l2_wide_redo"] + 1_000
    # the ballot search visits exactly the blocks the walk visits: the same windows scored and the same window states rebuilt, not only the same records
    zs, ws = res["zone"][3], res["walk"][3]
    assert zs["sum_l2_evals"] == ws["sum_l2_evals"] and zs["n_l2_rebuilds"] == ws["n_l2_rebuilds"], (zs, ws)
    # every block visit starts with a window-state rebuild and zone exits add more: more rebuilds than candidates that reach the sweep
    assert zs["n_l2_rebuilds"] > res["handback"][3]["n_l2_wide_redo"] - res["zone"][3]["n_l2_wide_redo"], zs
    for mode in ("zone", "walk", "handback", "zone_two_pass"):
        got = res[mode]
        assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1]), mode
        acc = base[2][:, 5] == 1
        assert np.array_equal(base[2][acc], got[2][acc]), mode
    idx.close(); reads.close(); ref.close()
