"""mm_gene_overlap (classify --genes on the device: interval join, per-group medians, per-read de-duplicated feature counts) through capi.py against the
Python restatement of its definition (tests/gene_ref.py).  Equality is exact: the counts are integers and a median is one of the inputs."""
import os

import numpy as np
import pytest

import gene_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def own_groups(n_genes, feats_per_group=0, n_feats=0):
    """every gene its own group; the group's features: feats_per_group consecutive ids"""
    foff = np.arange(n_genes + 1, dtype=np.int64) * feats_per_group
    feat = (np.arange(n_genes * feats_per_group) % max(n_feats, 1)).astype(np.int32)
    return np.arange(n_genes, dtype=np.int32), n_genes, foff, feat, n_feats


def run_and_check(ctx, table, maps, want=None):
    off, gs, ge, gg, n_groups, foff, feat, n_feats = table
    mc, ms, me, mi = maps
    got = ctx.gene_overlap(off, gs, ge, gg, n_groups, foff, feat, n_feats, mc, ms, me, mi)
    if want is None:
        want = gene_ref.overlap(off, gs, ge, gg, n_groups, foff, feat, n_feats, mc, ms, me, mi)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1], equal_nan=True)
    assert np.array_equal(got[2], want[2])
    assert got[3] == want[3]
    return got


def test_no_genes(ctx):
    empty = np.zeros(0, dtype=np.int32)
    maps = ([0, 1, 1], [5, 0, 9], [50, 7, 9], [0.9, 0.8, 0.7])
    got = run_and_check(ctx, ([0, 0, 0], empty, empty, empty, 0, [0], empty, 0), maps)
    assert len(got[0]) == 0 and got[3] == 0
    got = run_and_check(ctx, ([0, 0, 0], empty, empty, empty, 3, [0, 1, 1, 2], [1, 0], 2), maps)   # groups and features that no gene uses
    assert got[0].tolist() == [0, 0, 0] and np.all(np.isnan(got[1])) and got[2].tolist() == [0, 0]
    got = ctx.gene_overlap([0], empty, empty, empty, 0, [0], empty, 0, empty, empty, empty, np.zeros(0))   # no contig either
    assert got[3] == 0


def test_no_mappings(ctx):
    empty = np.zeros(0, dtype=np.int32)
    got = run_and_check(ctx, ([0, 2], [1, 5], [4, 9], [0, 1], 2, [0, 1, 2], [0, 1], 2), (empty, empty, empty, np.zeros(0)))
    assert got[0].tolist() == [0, 0] and np.all(np.isnan(got[1])) and got[2].tolist() == [0, 0] and got[3] == 0


@pytest.mark.parametrize("s,e,hit", [(0, 9, 0), (0, 10, 0), (0, 11, 1), (20, 30, 1), (21, 30, 0), (12, 15, 1), (5, 25, 1), (10, 10, 0), (20, 20, 1)])
def test_one_gene_one_mapping_boundary_relations(ctx, s, e, hit):
    """gene (10, 20): a mapping whose stop equals the gene's Start does not overlap it, one whose start equals the gene's Stop does"""
    got = run_and_check(ctx, ([0, 1], [10], [20], [0], 1, [0, 1], [0], 1), ([0], [s], [e], [0.875]))
    assert got[0].tolist() == [hit] and got[2].tolist() == [hit] and got[3] == 1
    assert (got[1][0] == 0.875) if hit else np.isnan(got[1][0])


def test_prefix_maximum_chain_as_long_as_the_contig(ctx):
    """3 000 genes under one gene that spans them all: pmax never falls below any mapping's start, the candidates of a mapping reach back to gene 0"""
    rng = np.random.default_rng(41)
    n = 3000
    gs = np.concatenate([[0], 100 + 30 * np.arange(n)]); ge = np.concatenate([[200_000], gs[1:] + rng.integers(5, 60, size=n)])
    ms = rng.integers(0, 95_000, size=2000); me = ms + rng.integers(0, 400, size=2000)
    table = ([0, n + 1], gs, ge) + own_groups(n + 1, 2, 50)
    got = run_and_check(ctx, table, (np.zeros(2000, dtype=np.int32), ms, me, rng.integers(800, 1000, size=2000) / 1000.0))
    assert got[0][0] == np.count_nonzero(me > 0) and got[0].sum() > 10_000


def test_lane_and_wavefront_walks_agree_across_the_split(ctx):
    """mappings that overlap exactly 63, 64, 65, 1 024 and 5 000 genes (and 1 and 0): a lane's walk up to 64 candidates, the wavefront's above"""
    n = 6000
    gs = 10 * np.arange(n); ge = gs + 5
    ks = [63, 64, 65, 1024, 5000, 1, 0, 64, 65, 2, 5000, 130]
    me = np.array([10 * (k - 1) + 1 if k else 0 for k in ks]); ms = np.zeros(len(ks), dtype=np.int64)
    ks2 = [63, 64, 65, 1024, 129]                                   # ... and the same counts away from the contig's first gene
    ms = np.concatenate([ms, np.full(len(ks2), 10 * 700)]); me = np.concatenate([me, [10 * (700 + k - 1) + 1 for k in ks2]])
    mi = (np.arange(len(ms)) % 5) / 8.0
    table = ([0, n], gs, ge) + own_groups(n, 1, 7)
    got = run_and_check(ctx, table, (np.zeros(len(ms), dtype=np.int32), ms, me, mi))
    assert got[0].sum() == sum(ks) + sum(ks2)
    for i, k in enumerate(ks[:5]):                                  # each alone (a wavefront with one wide mapping, or none)
        one = run_and_check(ctx, table, ([0], [0], [me[i]], [0.5]))
        assert one[0].sum() == k and one[0][:k].tolist() == [1] * k


def test_medians_of_groups_of_1_to_5_and_1000_identities_with_ties(ctx):
    sizes = [1, 2, 3, 4, 5, 1000]
    gs = 100 * np.arange(len(sizes)); ge = gs + 50
    rng = np.random.default_rng(42)
    mc, ms, mi = [], [], []
    for g, n in enumerate(sizes):
        ms += [gs[g] + 10] * n
        mi += (rng.integers(0, 7, size=n) / 16.0 + 0.5).tolist()     # seven distinct values: many ties
    order = rng.permutation(len(ms))
    ms, mi = np.array(ms)[order], np.array(mi)[order]
    table = ([0, len(sizes)], gs, ge) + own_groups(len(sizes))
    got = run_and_check(ctx, table, (np.zeros(len(ms), dtype=np.int32), ms, ms + 5, mi))
    assert got[0].tolist() == sizes
    for g, n in enumerate(sizes):
        x = np.sort(mi[(ms >= gs[g]) & (ms <= ge[g])])
        assert got[1][g] == x[(n - 1) // 2]
    zeros = run_and_check(ctx, table, (np.zeros(3, dtype=np.int32), [10, 10, 10], [15, 15, 15], [0.0, -0.0, 0.0]))   # -0.0 is 0
    assert zeros[1][0] == 0.0


def test_pooling_sharing_and_double_counting(ctx):
    # contig 0: genes A (10, 20) and B (15, 30); contig 1: gene A' (5, 9) in A's group; contig 0 also holds C (40, 50) and C' (45, 60), one group
    off, gs, ge = [0, 4, 5], [10, 15, 40, 45, 5], [20, 30, 50, 60, 9]
    gg, n_groups = [0, 1, 2, 2, 0], 3
    foff, feat, n_feats = [0, 2, 4, 5], [0, 1, 1, 2, 3], 4          # A: {0, 1}, B: {1, 2}, C: {3}
    maps = ([0, 1, 0, 0], [12, 6, 47, 100], [18, 8, 48, 110], [0.9, 0.7, 0.8, 0.6])
    got = run_and_check(ctx, (off, gs, ge, gg, n_groups, foff, feat, n_feats), maps)
    assert got[0].tolist() == [2, 1, 2]                             # A pooled over two contigs; the third read overlaps two intervals of C: counts twice
    assert got[1].tolist() == [0.7, 0.9, 0.8]                       # rank (2 - 1) // 2 = 0 of {0.7, 0.9}; of {0.8, 0.8}
    assert got[2].tolist() == [2, 2, 1, 1]                          # feature 1 is carried by A and B, both overlapped by read 0: counted once for it (and once for read 1)
    assert got[3] == 4


@pytest.fixture(scope="module")
def big():
    """100 000 mappings x 50 000 genes on 500 contigs (the last ten without genes); nested and overlapping genes; groups shared between contigs"""
    rng = np.random.default_rng(43)
    nc, per, L = 500, 102, 200_000
    off = np.concatenate([np.arange(nc - 9) * per, np.full(10, (nc - 10) * per)]).astype(np.int64)
    ng = int(off[-1])
    gs = np.sort(rng.integers(0, L, size=(nc - 10, per)), axis=1).ravel()
    ge = gs + rng.integers(300, 3000, size=ng)
    ge[::per] = L                                                   # every contig's first gene reaches its end
    gg = rng.integers(0, 40_000, size=ng)
    per_g = rng.integers(0, 8, size=40_000)
    foff = np.concatenate([[0], np.cumsum(per_g)])
    feat = np.where(rng.random(int(foff[-1])) < 0.3, rng.integers(0, 25, size=int(foff[-1])), rng.integers(0, 3000, size=int(foff[-1])))
    n = 100_000
    mc = rng.integers(0, nc, size=n); ms = rng.integers(0, L, size=n); me = ms + rng.integers(0, 10_000, size=n)
    mi = rng.integers(7000, 10001, size=n) / 100.0 / 100
    table = (off, gs, ge, gg, 40_000, foff, feat, 3000)
    maps = (mc, ms, me, mi)
    return table, maps, gene_ref.overlap(*table, *maps)


def test_100k_mappings_against_50k_genes(ctx, big):
    table, maps, want = big
    got = run_and_check(ctx, table, maps, want)
    assert got[0].sum() > 300_000 and np.count_nonzero(got[2]) > 2000 and 0 < got[3] < 100_000


def test_results_do_not_depend_on_the_tiling(ctx, big):
    table, maps, want = big
    pairs = int(want[0].sum())
    os.environ["MM_GENE_PAIR_BUDGET"] = str(pairs // 7)             # seven or more ranges of mappings, and of groups
    try:
        run_and_check(ctx, table, maps, want)
        os.environ["MM_GENE_PAIR_BUDGET"] = "3"                     # nearly every mapping is beyond the budget and a range of its own, hundreds of ranges of groups
        small = (table[0][:4],) + tuple(a[:int(table[0][3])] for a in table[1:4]) + table[4:]
        keep = maps[0] < 3
        run_and_check(ctx, small, tuple(a[keep] for a in maps))
    finally:
        del os.environ["MM_GENE_PAIR_BUDGET"]


def test_null_optional_outputs(ctx, big):
    table, maps, want = big
    sub = tuple(a[:5000] for a in maps)
    full = ctx.gene_overlap(*table, *sub)
    got = ctx.gene_overlap(*table, *sub, want_feats=False, want_annotated=False)
    assert got[2] is None and got[3] is None
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1], equal_nan=True)


GOOD = dict(off=[0, 2, 3], gs=[5, 5, 1], ge=[9, 5, 1], gg=[0, 1, 1], n_groups=2, foff=[0, 2, 3], feat=[3, 0, 1], n_feats=4,
            mc=[0, 1], ms=[1, 7], me=[5, 7], mi=[0.9, 0.0])


@pytest.mark.parametrize("change,word", [(dict(off=[1, 2, 3]), "contig_gene_off"), (dict(off=[0, 3, 2]), "contig_gene_off"), (dict(gs=[5, 4, 1]), "sorted by Start"),
                                         (dict(ge=[9, 4, 1]), "Stop"), (dict(gg=[0, 2, 1]), "gene_group"), (dict(gg=[0, -1, 1]), "gene_group"),
                                         (dict(foff=[0, 2, 1], feat=[3, 0]), "group_feat_off"), (dict(feat=[3, 4, 1]), "feature id"), (dict(feat=[3, -1, 1]), "feature id"),
                                         (dict(mc=[0, 2]), "map_contig"), (dict(mc=[-1, 1]), "map_contig"), (dict(ms=[6, 7]), "map_stop"),
                                         (dict(mi=[-0.5, 0.0]), "identity"), (dict(mi=[0.9, float("nan")]), "identity")])
def test_refusals(ctx, change, word):
    from metamaps_amd import capi
    a = dict(GOOD, **change)
    args = (a["off"], a["gs"], a["ge"], a["gg"], a["n_groups"], a["foff"], a["feat"], a["n_feats"], a["mc"], a["ms"], a["me"], a["mi"])
    with pytest.raises(capi.MMError) as e:
        ctx.gene_overlap(*args)
    assert e.value.status == -1 and word in str(e.value), str(e.value)
    g = GOOD
    run_and_check(ctx, (g["off"], g["gs"], g["ge"], g["gg"], g["n_groups"], g["foff"], g["feat"], g["n_feats"]), (g["mc"], g["ms"], g["me"], g["mi"]))   # the context still works
