"""mm_em_lca: the confidence-thresholded LCA assignment on the device against the Python restatement of its definition (tests/lca_ref.py).
Exact problems: n_taxa a power of two, f uniform, inv_nloc 1 and mapq multiples of 2^-20 that sum to 1 per read, so the posteriors are the
mapq, every mass is exact, and node, mass and the direct counts must match exactly, also where a mass equals the threshold."""
import numpy as np
import pytest

import lca_ref

pytestmark = pytest.mark.gpu
LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 5000]      # (15-17: the step from a group of lanes per read to the whole wavefront)


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def exact_problem(rng, parent, lens, n_taxa=64, clustered=0.5):
    """taxa on leaves and internal nodes; a read's entries on any taxa, or (clustered) on the taxa below a random node where there are some"""
    n = len(parent)
    taxon_node = rng.integers(0, n, size=n_taxa).astype(np.int32)
    depth = lca_ref.depths(parent)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    taxon, mapq = [], []
    for k in lens:
        if k == 0:
            continue
        pool = np.arange(n_taxa)
        if rng.random() < clustered:
            top = int(taxon_node[rng.integers(0, n_taxa)])
            for _ in range(int(rng.integers(0, 3))):
                top = int(parent[top])
            a = taxon_node.astype(np.int64).copy()
            while (depth[a] > depth[top]).any():
                a = np.where(depth[a] > depth[top], parent[a], a)
            pool = np.flatnonzero(a == top)
        taxon.append(rng.choice(pool, size=k))
        mapq.append(lca_ref.exact_posteriors(rng, k))
    taxon = np.concatenate(taxon).astype(np.int32) if taxon else np.zeros(0, dtype=np.int32)
    mapq = np.concatenate(mapq) if mapq else np.zeros(0)
    return off, taxon, mapq, taxon_node


def run(ctx, parent, off, taxon, mapq, taxon_node, tau, **kw):
    n_taxa = len(taxon_node)
    em = ctx.em(off, taxon, mapq, np.ones(len(taxon)), n_taxa)
    try:
        return em.lca(np.full(n_taxa, 1.0 / n_taxa), parent, taxon_node, tau, **kw)
    finally:
        em.close()


def check(ctx, parent, off, taxon, mapq, taxon_node, taus):
    for tau in taus:
        node, mass, direct = run(ctx, parent, off, taxon, mapq, taxon_node, tau)
        want = lca_ref.assign(parent, off, taxon_node[taxon], mapq, tau)
        bad = np.flatnonzero((node != want[0]) | (mass != want[1]))
        assert len(bad) == 0, (tau, bad[:5], node[bad[:5]], want[0][bad[:5]], mass[bad[:5]], want[1][bad[:5]], np.diff(off)[bad[:5]])
        assert np.array_equal(direct, want[2]), tau
        assert direct.sum() == np.count_nonzero(np.diff(off))


@pytest.mark.parametrize("shape,n_nodes", [("random", 300), ("deep", 120), ("chain", 41), ("root", 1), ("random", 4096), ("random", 4097)])
def test_every_read_length_in_one_problem(ctx, shape, n_nodes):
    """all the lengths at which the kernel changes its path, shuffled, on trees in LDS (up to 4096 nodes) and one just beyond"""
    rng = np.random.default_rng(31 + n_nodes)
    parent = np.zeros(1, dtype=np.int32) if shape == "root" else lca_ref.random_tree(rng, n_nodes, shape)
    lens = np.array(LENS * 3 + [1, 2, 3] * 20)
    rng.shuffle(lens)
    off, taxon, mapq, taxon_node = exact_problem(rng, parent, lens.tolist())
    check(ctx, parent, off, taxon, mapq, taxon_node, (0.51, 0.8, 1.0))


def test_one_read(ctx):
    rng = np.random.default_rng(32)
    parent = lca_ref.random_tree(rng, 50, "random")
    for k in (1, 7, 200):
        off, taxon, mapq, taxon_node = exact_problem(rng, parent, [k])
        check(ctx, parent, off, taxon, mapq, taxon_node, (0.51, 0.75))


@pytest.fixture(scope="module")
def large():
    """100 000 reads on a tree of 50 000 nodes (read from global memory), 4 096 taxa"""
    rng = np.random.default_rng(33)
    parent = lca_ref.random_tree(rng, 50_000, "random")
    n_taxa, n_reads = 4096, 100_000
    taxon_node = rng.integers(0, len(parent), size=n_taxa).astype(np.int32)
    lens = rng.integers(0, 9, size=n_reads)
    lens[rng.integers(0, n_reads, size=40)] = rng.integers(17, 400, size=40)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ne = int(off[-1])
    # entries of a read on a run of neighbouring taxa (sorted by the tin order of their nodes they would be relatives; random ones are not: both occur)
    base = np.repeat(rng.integers(0, n_taxa, size=n_reads), lens)
    taxon = ((base + rng.integers(0, 4, size=ne) * (rng.random(ne) < 0.7)) % n_taxa).astype(np.int32)
    k = rng.integers(1, 1 << 11, size=ne).astype(np.int64)            # multiples of 2^-20 that sum to 1: the last entry of a read takes the rest (400 * 2^11 < 2^20)
    rd = np.repeat(np.arange(n_reads), lens)
    last = off[1:][lens > 0] - 1
    k[last] = 0
    s = np.bincount(rd, weights=k, minlength=n_reads).astype(np.int64)
    k[last] = (1 << 20) - s[lens > 0]
    assert (k > 0).all()
    mapq = k.astype(np.float64) / float(1 << 20)
    return parent, off, taxon, mapq, taxon_node


def test_100000_reads_on_a_tree_beyond_lds(ctx, large):
    parent, off, taxon, mapq, taxon_node = large
    check(ctx, parent, off, taxon, mapq, taxon_node, (0.8,))


def test_cut_in_two_at_a_read_boundary(ctx, large):
    parent, off, taxon, mapq, taxon_node = large
    n = 20_000
    off, taxon, mapq = off[:n + 1], taxon[:off[n]], mapq[:off[n]]
    whole = run(ctx, parent, off, taxon, mapq, taxon_node, 0.75)
    cut, e = 7_777, int(off[7_777])
    a = run(ctx, parent, off[:cut + 1], taxon[:e], mapq[:e], taxon_node, 0.75)
    b = run(ctx, parent, off[cut:] - e, taxon[e:], mapq[e:], taxon_node, 0.75)
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0]) and np.array_equal(np.concatenate([a[1], b[1]]), whole[1])
    assert np.array_equal(a[2] + b[2], whole[2])


def test_constructed_reads(ctx):
    """0 - 1 - {2 - 4, 3}: taxon t sits on node t (taxa 5-7 on the root)"""
    parent = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    taxon_node = np.array([0, 1, 2, 3, 4, 0, 0, 0], dtype=np.int32)
    reads = [([4, 4, 4], [0.25, 0.5, 0.25]),                       # all entries on one taxon
             ([2, 3], [0.5, 0.5]),                                 # two taxa at 0.5 / 0.5 under a common parent
             ([2, 3], [0.75, 0.25]),                               # mass equal to the threshold at a node (0.75)
             ([2, 4], [0.25, 0.75]),                               # a taxon that is an ancestor of another taxon of the read
             ([4, 3, 0], [0.75, 0.125, 0.125]),
             ([], [])]
    off = np.concatenate([[0], np.cumsum([len(t) for t, _ in reads])]).astype(np.int64)
    taxon = np.array(sum((t for t, _ in reads), []), dtype=np.int32)
    mapq = np.array(sum((p for _, p in reads), []), dtype=np.float64)
    want = {0.51: ([4, 1, 2, 4, 4, -1], [1.0, 1.0, 0.75, 0.75, 0.75, 0.0]),
            0.75: ([4, 1, 2, 4, 4, -1], [1.0, 1.0, 0.75, 0.75, 0.75, 0.0]),
            0.8: ([4, 1, 1, 2, 1, -1], [1.0, 1.0, 1.0, 1.0, 0.875, 0.0]),
            1.0: ([4, 1, 1, 2, 0, -1], [1.0, 1.0, 1.0, 1.0, 1.0, 0.0])}
    for tau, (nodes, masses) in want.items():
        node, mass, direct = run(ctx, parent, off, taxon, mapq, taxon_node, tau)
        assert node.tolist() == nodes and mass.tolist() == masses, (tau, node, mass)
        assert direct.tolist() == np.bincount([v for v in nodes if v >= 0], minlength=5).tolist()
    check(ctx, parent, off, taxon, mapq, taxon_node, tuple(want))


def test_refusals_and_optional_outputs(ctx):
    from metamaps_amd import capi
    rng = np.random.default_rng(34)
    parent = lca_ref.random_tree(rng, 30, "random")
    off, taxon, mapq, taxon_node = exact_problem(rng, parent, [3, 0, 20, 1])
    full = run(ctx, parent, off, taxon, mapq, taxon_node, 0.8)
    node, mass, direct = run(ctx, parent, off, taxon, mapq, taxon_node, 0.8, want_mass=False, want_direct=False)
    assert mass is None and direct is None and np.array_equal(node, full[0])
    node, mass, direct = run(ctx, parent, off, taxon, mapq, taxon_node, 0.8, want_mass=False)
    assert mass is None and np.array_equal(direct, full[2])
    bad_parent = [np.array([1, 0], dtype=np.int32), np.array([0, 0, 2], dtype=np.int32), np.array([0, 0, 3, 1], dtype=np.int32), np.array([0, -1], dtype=np.int32)]
    out_of_tree = [np.where(np.arange(len(taxon_node)) == 5, v, taxon_node).astype(np.int32) for v in (-1, len(parent))]
    cases = [(parent, taxon_node, tau) for tau in (0.5, 0.509, 1.0000001, 0.0, -0.8, float("nan"), float("inf"))]
    cases += [(p, np.zeros_like(taxon_node), 0.8) for p in bad_parent] + [(parent, t, 0.8) for t in out_of_tree]
    for p, t, tau in cases:
        with pytest.raises(capi.MMError) as e:
            run(ctx, p, off, taxon, mapq, t, tau)
        assert e.value.status == -1, (p, t, tau)


def test_posteriors_of_a_real_em(ctx):
    """non-uniform f after mm_em_run: the masses are recomputed from mm_em_posteriors' doubles; a read is left out only if one of its node
    masses lies within 1e-9 of tau - 1e-9 (the expected share of such reads is of the order of 1e-8)"""
    rng = np.random.default_rng(35)
    parent = lca_ref.random_tree(rng, 400, "random")
    n_taxa, n_reads, tau = 128, 20_000, 0.8
    taxon_node = rng.integers(0, len(parent), size=n_taxa).astype(np.int32)
    lens = rng.integers(1, 7, size=n_reads)
    lens[rng.integers(0, n_reads, size=10)] = rng.integers(17, 300, size=10)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ne = int(off[-1])
    ab = rng.lognormal(0, 1.5, size=n_taxa)
    base = np.repeat(rng.choice(n_taxa, size=n_reads, p=ab / ab.sum()), lens)
    taxon = ((base + rng.integers(0, 3, size=ne)) % n_taxa).astype(np.int32)
    mapq = rng.uniform(0.05, 1.0, size=ne)
    inv = 1.0 / rng.integers(1000, 9000, size=ne).astype(np.float64)
    em = ctx.em(off, taxon, mapq, inv, n_taxa)
    try:
        f, _ = em.run(np.full(n_taxa, 1.0 / n_taxa))
        assert f.max() > 4 * f[f > 0].min()                         # not uniform
        post, _ = em.posteriors(f)
        node, mass, direct = em.lca(f, parent, taxon_node, tau)
    finally:
        em.close()
    want_node, want_mass, _, near = lca_ref.assign(parent, off, taxon_node[taxon], post, tau, margin=1e-9)
    print(f"reads left out: {int(near.sum())} of {n_reads}")
    assert near.mean() <= 0.001
    keep = ~near
    assert np.array_equal(node[keep], want_node[keep])
    assert np.allclose(mass[keep], want_mass[keep], rtol=0, atol=1e-12)   # (sums of at most 300 doubles in another order)
    assert np.array_equal(direct, np.bincount(node, minlength=len(parent)))
    assert len(np.unique(node)) > 20 and (node == taxon_node[taxon[off[:-1]]]).mean() < 0.9   # (not every read on its first taxon)
