"""The bootstrap EM (mm_em_bootstrap: boot_p1 / p2 / p3_kernel and boot_run, mm_boot.hip) at its edges, against the exact weighted host EM of
tests/post_ref.py on the cases of tests/boot_cases.py (checked on the CPU by tests/test_boot_cases.py): reads without a mapping before, between
and after the mapped ones (the weights' read index is not the read index), the 8-mapping chunks of P1b, the 512-entry items of P2b, P3b's 16
rows, tiles of 64 replicates that stop in different iterations, max_iter at the edges of boot_run's groups, replicate numbers up to 2^31 - 1,
and replicates that draw no read.  Bounds as for the point loop (test_gpu_post_edges.py::test_em_loop_against_host_reference)."""
import numpy as np
import pytest

import boot_cases as bc
from test_gpu_post_edges import K, LOOP_PROBLEMS, WINDOW, records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def device_em(ctx, name):
    off, taxon, mapq, inv, T = bc.problem(name)
    return ctx.em(off, taxon, mapq, inv, T)


def absent_taxa(name):
    _, taxon, _, _, T = bc.problem(name)
    return np.bincount(taxon, minlength=T) == 0


def check_row(got, k, want, absent, what):
    """row k of a call's four outputs against the reference's (f, ll, n_iter, stopped, margins)"""
    fb, llb, itb, stb = got
    f, ll, n_iter, stopped, _ = want
    assert itb[k] == n_iter and bool(stb[k]) == stopped, (what, int(itb[k]), n_iter, bool(stb[k]), stopped)
    if n_iter == 0:                                                 # an empty weighted sample
        assert not fb[k].any() and llb[k] == 0 and stb[k], what
        return
    assert abs(llb[k] - ll) <= 1e-12 * abs(ll), (what, llb[k], ll)
    assert np.allclose(fb[k], f, rtol=1e-10, atol=1e-300), (what, np.max(np.abs(fb[k] - f)))
    assert np.all(fb[k][absent] == 0), what


def all_finite(got):
    return all(np.all(np.isfinite(a)) for a in got[:2])


def same_rows(a, rows_a, b, rows_b):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in range(4))


# ----------------------------------------------------------------------------------------------------------------------------------
# unit weights: the point EM
# ----------------------------------------------------------------------------------------------------------------------------------
def check_unit_weights(e, f0, n_mapped):
    f_pt, lls = e.run(f0, max_iter=1000)
    assert 0 < len(lls) < 1000
    got = e.bootstrap(f0, 4, seed=1, weights=np.ones((4, n_mapped), dtype=np.uint8), max_iter=1000)
    fb, llb, itb, stb = got
    assert all_finite(got) and stb.all()
    for r in range(4):
        assert itb[r] == len(lls)
        np.testing.assert_allclose(fb[r], f_pt, rtol=1e-12, atol=1e-300)
        assert abs(llb[r] - lls[-1]) <= 1e-12 * abs(lls[-1])


@pytest.mark.parametrize("name", list(LOOP_PROBLEMS))
def test_unit_weights_equal_the_point_em(ctx, name):
    e = device_em(ctx, name)
    check_unit_weights(e, bc.f_start(name), bc.mapped_reads(name))
    e.close()


def test_unit_weights_on_the_window_of_tiny_qualities(ctx):
    """the problem of test_window_of_tiny_qualities_does_not_poison_the_em: qualities in (0, 1e-303) in every replicate, no NaN in any"""
    from metamaps_amd import capi
    rl, off, rec = records([WINDOW])
    n = len(rec)
    M = capi.Mapping.from_parts(ctx, rl, [(off, rec)], [0], K, 8)
    M.add_qualities(K)
    e = ctx.em_from_mapping(M, np.arange(n), np.full(n, 50_000), n)
    check_unit_weights(e, np.full(n, 1.0 / n), 1)
    e.close(); M.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# generated and caller weights against the weighted reference
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.GENERATED)
def test_generated_weights_against_host_reference(ctx, name):
    e = device_em(ctx, name)
    got = e.bootstrap(bc.f_start(name), bc.GENERATED_B, seed=bc.SEED)
    e.close()
    assert all_finite(got)
    absent = absent_taxa(name)
    for r in bc.GENERATED_REPS + tuple(bc.MARKED.get(name, ())):
        check_row(got, r, bc.expected(name, r), absent, (name, r))
    empty = bc.empty_replicates(name, bc.GENERATED_B)
    for r in range(bc.GENERATED_B):                                 # the other replicates: an estimate each (their bits: the identities of the tile test)
        assert (got[2][r] == 0) == (r in empty) and abs(got[0][r].sum() - (r not in empty)) < 1e-12 and np.all(got[0][r][absent] == 0), (name, r)


def test_caller_weights_against_host_reference(ctx):
    name = "mappings_per_read"
    w = bc.caller_rows(name)
    assert w.shape == (4, bc.mapped_reads(name)) and w[1].tolist() == [1] * w.shape[1] and {0, 1, 2, 255} == set(w[[0, 2, 3]].ravel().tolist())
    e = device_em(ctx, name)
    got = e.bootstrap(bc.f_start(name), 4, seed=1, weights=w)
    e.close()
    assert all_finite(got)
    for k in range(4):
        check_row(got, k, bc.expected(name, None, "rows", k), absent_taxa(name), (name, "row", k))


# ----------------------------------------------------------------------------------------------------------------------------------
# tiles of 64 replicates whose lanes freeze in different iterations
# ----------------------------------------------------------------------------------------------------------------------------------
def test_tiles_and_freezing(ctx):
    name = bc.TILE
    f0 = bc.f_start(name)
    e = device_em(ctx, name)
    calls = {B: e.bootstrap(f0, B, seed=bc.SEED) for B in bc.TILE_B}
    whole = calls[129]
    assert all_finite(whole) and whole[3].all() and len(set(whole[2][:65].tolist())) >= 3
    for B in bc.TILE_B:                                             # a row does not depend on the replicates of its call
        assert same_rows(calls[B], slice(0, B), whole, slice(0, B)), B
    for n_first in (1, 64, 63):                                     # nor on how 65 replicates are split over calls
        a = e.bootstrap(f0, n_first, seed=bc.SEED)
        b = e.bootstrap(f0, 65 - n_first, seed=bc.SEED, rep0=n_first)
        assert same_rows(a, slice(0, n_first), whole, slice(0, n_first)) and same_rows(b, slice(0, 65 - n_first), whole, slice(n_first, 65)), n_first
    absent = absent_taxa(name)
    for r in bc.tile_reps():                                        # 0, 63, 64, the earliest and the latest stopper: alone, and against the reference
        alone = e.bootstrap(f0, 1, seed=bc.SEED, rep0=r)
        assert same_rows(alone, slice(0, 1), whole, slice(r, r + 1)), r
        check_row(whole, r, bc.expected(name, r), absent, (name, r))
    e.close()


@pytest.mark.parametrize("cap", bc.CAPS)
def test_max_iter_at_the_group_edges(ctx, cap):
    """boot_run enqueues 24 iterations, then eights: a limit inside, at the end of and just behind a group"""
    name = "slow"
    e = device_em(ctx, name)
    got = e.bootstrap(bc.f_start(name), bc.CAP_B, seed=bc.SEED, max_iter=cap)
    e.close()
    assert all_finite(got)
    full = bc.iterations(name, range(bc.CAP_B))
    for r in range(bc.CAP_B):
        check_row(got, r, bc.expected(name, r, None, None, cap), absent_taxa(name), (name, r, cap))
        assert bool(got[3][r]) == (full[r] <= cap) and got[2][r] == min(full[r], cap)


def test_replicate_numbers_up_to_the_last(ctx):
    from metamaps_amd import capi
    name = bc.BIG
    e = device_em(ctx, name)
    got = e.bootstrap(bc.f_start(name), bc.BIG_N, seed=bc.SEED, rep0=bc.BIG_REP0)
    assert all_finite(got) and got[3].all()
    for r in bc.BIG_REPS:
        check_row(got, r - bc.BIG_REP0, bc.expected(name, r), absent_taxa(name), (name, r))
    assert not np.array_equal(got[0][0], got[0][bc.BIG_N - 1])
    with pytest.raises(capi.MMError) as ei:
        e.bootstrap(bc.f_start(name), bc.BIG_N, seed=bc.SEED, rep0=bc.BIG_REP0 + 1)
    assert ei.value.status == -1
    e.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# replicates that draw no read
# ----------------------------------------------------------------------------------------------------------------------------------
def test_empty_replicates_report_no_estimate_and_cost_no_iterations(ctx):
    name, B = bc.EMPTY, bc.EMPTY_B
    empty = bc.empty_replicates(name, B)
    assert empty == [7, 18, 54, 69, 86, 126]
    e = device_em(ctx, name)
    got = e.bootstrap(bc.f_start(name), B, seed=bc.SEED, max_iter=10_000)
    fb, llb, itb, stb = got
    assert all_finite(got)                                          # no NaN, no inf anywhere
    assert [r for r in range(B) if itb[r] == 0] == empty            # (10 000 iterations each, were they run to the limit)
    for r in range(B):
        check_row(got, r, bc.expected(name, r), absent_taxa(name), (name, r))
    for r in empty:
        assert not fb[r].any() and llb[r] == 0 and itb[r] == 0 and stb[r]
    for r in (6, 8, 53, 55, 127):                                   # their neighbours are what they are without them
        alone = e.bootstrap(bc.f_start(name), 1, seed=bc.SEED, rep0=r)
        assert same_rows(alone, slice(0, 1), got, slice(r, r + 1)), r
    e.close()


def test_a_problem_without_mappings_has_only_empty_replicates(ctx):
    name = "no_mapping"
    e = device_em(ctx, name)
    T = bc.problem(name)[4]
    for weights in (None, np.zeros((5, 0), dtype=np.uint8)):
        fb, llb, itb, stb = e.bootstrap(bc.f_start(name), 5, seed=bc.SEED, weights=weights)
        assert fb.tolist() == [[0.0] * T] * 5 and llb.tolist() == [0.0] * 5 and itb.tolist() == [0] * 5 and stb.all()
    e.close()


def test_a_caller_row_of_zeros_between_rows_of_ones(ctx):
    name = bc.EMPTY
    e = device_em(ctx, name)
    got = e.bootstrap(bc.f_start(name), 3, seed=1, weights=bc.zero_row_between_ones(name))
    assert all_finite(got)
    for k in range(3):
        check_row(got, k, bc.expected(name, None, "zero_row", k), absent_taxa(name), (name, "zero_row", k))
    assert got[2][1] == 0 and got[2][0] > 0 and same_rows(got, slice(0, 1), got, slice(2, 3))
    ones = e.bootstrap(bc.f_start(name), 1, seed=1, weights=np.ones((1, 3), dtype=np.uint8))
    assert same_rows(ones, slice(0, 1), got, slice(0, 1))
    e.close()
