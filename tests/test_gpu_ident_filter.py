"""mm_ident_filter (classify --min-identity on the device: every read's largest identity, the genomes' median best identities, the removed genomes and
the EM problem without them) through capi.py against the naive restatement of its definition (tests/ident_ref.py).  Equality is exact: every result is
an integer or a double selected from the input."""
import numpy as np
import pytest

import ident_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def run_and_check(ctx, off, taxon, ident, best, n_taxa, thr, want=None):
    got = ctx.ident_filter(off, taxon, ident, best, n_taxa, thr)
    if want is None:
        want = ident_ref.filter_arrays(off, taxon, ident, best, n_taxa, thr)
    ident_ref.same(got, want)
    flat = ctx.ident_filter(off, taxon, ident, best, n_taxa, thr, want_filtered=False)     # the filtered problem's outputs NULL as a group
    ident_ref.same(flat, want, filtered=False)
    assert flat["read_src"] is None
    # the filtered problem is consistent in itself
    rs, es, ro = got["read_src"], got["entry_src"], got["read_off_out"]
    off = np.asarray(off, dtype=np.int64)
    assert np.all(np.diff(rs) > 0) and np.all(np.diff(es) > 0) and len(ro) == len(rs) + 1 and ro[0] == 0 and ro[-1] == len(es) and np.all(np.diff(ro) > 0)
    for k in range(min(len(rs), 200)):
        mine = es[ro[k]:ro[k + 1]]
        assert off[rs[k]] <= mine[0] and mine[-1] < off[rs[k] + 1]
    return got


def one_entry_reads(taxon, ident):
    n = len(taxon)
    return (np.arange(n + 1), taxon, ident, np.arange(n))


def test_zero_reads_and_only_empty_reads(ctx):
    e = np.zeros(0)
    got = run_and_check(ctx, [0], e, e, e, 3, 80.0)
    assert len(got["sorted_max"]) == 0 and got["read_off_out"].tolist() == [0] and np.all(np.isnan(got["taxon_median"]))
    got = run_and_check(ctx, [0, 0, 0, 0], e, e, [0, 7, -1], 3, 80.0)
    assert len(got["sorted_max"]) == 0 and not got["read_removed"].any() and got["read_off_out"].tolist() == [0]
    got = run_and_check(ctx, [0], e, e, e, 0, 80.0)                # no taxon either
    assert got["n_le"] == 0


def test_one_read_with_one_entry(ctx):
    got = run_and_check(ctx, [0, 1], [0], [85.5], [0], 1, 80.0)
    assert got["sorted_max"].tolist() == [85.5] and got["taxon_median"].tolist() == [85.5] and got["entry_src"].tolist() == [0]
    got = run_and_check(ctx, [0, 1], [0], [85.5], [0], 1, 90.0)
    assert got["read_removed"].tolist() == [True] and len(got["read_src"]) == 0 and got["n_le"] == 1


def test_upper_medians_of_1_to_5_and_a_taxon_without_reads(ctx):
    sizes = [1, 2, 3, 4, 5]                                         # ranks 0, 1, 1, 2, 2
    tx = np.repeat(np.arange(5), sizes)
    idn = np.concatenate([10.0 * t + np.arange(n)[::-1] for t, n in enumerate(sizes)])
    order = np.random.default_rng(61).permutation(len(tx))
    got = run_and_check(ctx, *one_entry_reads(tx[order], idn[order]), 6, 25.0)
    assert got["taxon_median"][:5].tolist() == [0.0, 11.0, 21.0, 32.0, 42.0] and np.isnan(got["taxon_median"][5])
    assert got["taxon_removed"].tolist() == [True, True, True, False, False, False] and got["taxon_reads"].tolist() == sizes + [0]


def test_median_equal_to_the_threshold_stays(ctx):
    below = np.nextafter(80.0, 0)
    got = run_and_check(ctx, *one_entry_reads([0, 0, 0, 1, 1, 1], [70, 80, 90, 70, below, 90]), 2, 80.0)
    assert got["taxon_median"].tolist() == [80.0, below] and got["taxon_removed"].tolist() == [False, True]
    assert got["n_le"] == 4                                         # 70, 70, the double below 80, and 80 itself (<=)


def test_all_identities_equal_and_negative_zero(ctx):
    got = run_and_check(ctx, *one_entry_reads([0, 1, 0, 1], [77.5] * 4), 2, 77.5)
    assert not got["taxon_removed"].any() and got["n_le"] == 4
    got = run_and_check(ctx, *one_entry_reads([0, 0, 0], [0.0, -0.0, 0.0]), 1, 0.0)
    assert not np.signbit(got["sorted_max"]).any() and not np.signbit(got["taxon_median"]).any() and got["n_le"] == 3


def test_largest_identity_is_not_the_best_entrys(ctx):
    got = run_and_check(ctx, [0, 2, 4], [0, 1, 1, 0], [99.0, 60.0, 50.0, 95.0], [1, 2], 2, 80.0)
    assert got["sorted_max"].tolist() == [95.0, 99.0] and got["taxon_reads"].tolist() == [0, 2] and got["taxon_median"][1] == 60.0
    assert got["read_removed"].all() and got["read_src"].tolist() == [0, 1] and got["entry_src"].tolist() == [0, 3]   # both lose their best and keep an entry


@pytest.mark.parametrize("thr,all_gone", [(0.0, False), (100.0, True), (150.0, True), (float("inf"), True), (-5.0, False)])
def test_thresholds_that_remove_nothing_or_everything(ctx, thr, all_gone):
    got = run_and_check(ctx, *one_entry_reads([0, 1, 2, 2], [10.0, 50.0, 99.0, 99.5]), 3, thr)
    assert got["taxon_removed"].all() == all_gone and got["taxon_removed"].any() == all_gone
    assert len(got["read_src"]) == (0 if all_gone else 4) and got["n_le"] == (4 if all_gone else 0)


def test_reads_on_both_sides_of_the_group_and_the_wavefront(ctx):
    """reads of 16, 17, 64, 65 and 1 000 entries among one-entry reads: a group of 16 lanes up to 16 entries, the whole wavefront above; the largest identity
    sits at the read's last entry, at its first, and in the middle"""
    rng = np.random.default_rng(62)
    sizes = []
    for n in [16, 17, 64, 65, 1000, 15, 33, 16, 17, 1000, 129]:
        sizes += [1] * int(rng.integers(0, 7)) + [n]
    sizes += [1, 1, 0, 1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    ne = int(off[-1])
    taxon = rng.integers(0, 9, size=ne)
    ident = rng.integers(6000, 9000, size=ne) / 100.0
    for k, r in enumerate(np.flatnonzero(np.array(sizes) > 1)):
        ident[[off[r + 1] - 1, off[r], (off[r] + off[r + 1]) // 2][k % 3]] = 95.0 + k / 16.0
    best = np.array([rng.integers(off[r], off[r + 1]) if sizes[r] else -1 for r in range(len(sizes))])
    got = run_and_check(ctx, off, taxon, ident, best, 9, 75.0)
    assert got["sorted_max"][-11:].tolist() == [95.0 + k / 16.0 for k in range(11)]
    assert 0 < got["taxon_removed"].sum() < 9


@pytest.fixture(scope="module")
def big():
    """70 000 reads (more than 65 536; several hundred workgroups) of 0 to 5 entries, a few of 40, over 300 taxa of random sizes; identities in hundredths"""
    rng = np.random.default_rng(63)
    nr = 70_000
    sizes = rng.choice([0, 1, 1, 1, 2, 3, 5], size=nr)
    sizes[rng.integers(0, nr, size=50)] = 40
    off = np.concatenate([[0], np.cumsum(sizes)])
    ne = int(off[-1])
    w = rng.dirichlet(np.full(300, 0.3))
    taxon = rng.choice(300, size=ne, p=w)
    level = rng.uniform(70, 99, size=300)                           # every taxon has its own level of identity
    ident = np.round(np.clip(level[taxon] + rng.normal(0, 3, size=ne), 0, 100), 2)
    best = np.where(sizes > 0, off[:-1] + rng.integers(0, 1 << 30, size=nr) % np.maximum(sizes, 1), -1)
    p = (off, taxon, ident, best, 300, 85.0)
    return p, ident_ref.filter_arrays(*p)


def test_70000_reads_over_300_taxa(ctx, big):
    p, want = big
    got = run_and_check(ctx, *p, want=want)
    assert 50 < got["taxon_removed"].sum() < 250 and 1000 < len(got["read_src"]) < np.count_nonzero(np.diff(p[0]))
    lost_some = np.diff(got["read_off_out"]) < np.diff(p[0])[got["read_src"]]
    assert lost_some.any() and not lost_some.all()


def test_70000_reads_in_one_taxon(ctx, big):
    (off, taxon, ident, best, _, _), _ = big
    one = np.zeros(len(taxon), dtype=np.int32)
    for thr in (85.0, 60.0):
        got = run_and_check(ctx, off, one, ident, best, 1, thr)
    assert got["taxon_reads"][0] == np.count_nonzero(np.diff(off)) and not got["taxon_removed"][0]


GOOD = dict(off=[0, 2, 3], taxon=[0, 1, 1], ident=[90.0, 80.0, 70.0], best=[1, 2], n_taxa=2, thr=80.0)


@pytest.mark.parametrize("change,word", [(dict(off=[1, 2, 3]), "read_off"), (dict(off=[0, 3, 2]), "read_off"), (dict(taxon=[0, 2, 1]), "taxon"), (dict(taxon=[0, -1, 1]), "taxon"),
                                         (dict(best=[2, 2]), "best"), (dict(best=[0, 1]), "best"), (dict(best=[-1, 2]), "best"),
                                         (dict(ident=[90.0, -0.5, 70.0]), "identity"), (dict(ident=[90.0, float("nan"), 70.0]), "identity"),
                                         (dict(thr=float("nan")), "threshold")])
def test_refusals_leave_the_outputs_untouched(ctx, change, word):
    from metamaps_amd import capi
    a = dict(GOOD, **change)
    with pytest.raises(capi.MMError) as e:
        ctx.ident_filter(a["off"], a["taxon"], a["ident"], a["best"], a["n_taxa"], a["thr"])
    assert e.value.status == -1 and word in str(e.value), str(e.value)
    o = e.value.outputs                                             # as capi handed them in: -1, 255
    for k in ("sorted_max", "taxon_reads", "taxon_median", "read_src", "entry_src", "read_off_out"):
        assert np.all(o[k] == -1), k
    assert np.all(o["taxon_removed"] == 255) and np.all(o["read_removed"] == 255)
    assert o["n_with_entries"] == o["n_le"] == o["n_reads_out"] == o["n_entries_out"] == -1
    g = GOOD
    run_and_check(ctx, g["off"], g["taxon"], g["ident"], g["best"], g["n_taxa"], g["thr"])   # the context still works
