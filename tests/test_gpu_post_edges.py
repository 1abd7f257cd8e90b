"""K8 (mapping qualities) and K9 (EM problem from records, the per-call kernels, the device-resident loop) at their edges, against references
that share no code with them (tests/post_ref.py): exact binomial masses (mpmath) for K8, a float64 host EM with exact sums for K9.  Every
problem is built here from fixed seeds: records enter through Mapping.from_parts, EM problems through Context.em — no index, no mapping run,
no oracle.  The shapes follow the rules of em_grid, em_p1 and em_prepare (mm_post.hip), restated where a test leans on them."""
import math

import mpmath
import numpy as np
import pytest

import post_ref

pytestmark = pytest.mark.gpu

K = 16
EM_LBUF, EM_RBUF, EM_ITEM = 512, 192, 512                          # P1's LDS block (mappings, reads), P2's item: mm_post.hip


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# K8
# ----------------------------------------------------------------------------------------------------------------------------------
def records(reads, contig_of=None):
    """reads: [(length, sketch, [shared, ...])] -> (read_len, offsets, records) for Mapping.from_parts; record i lies on contig contig_of(i)"""
    from metamaps_amd import capi
    off = np.concatenate([[0], np.cumsum([len(sh) for _, _, sh in reads])]).astype(np.int64)
    rec = np.zeros(int(off[-1]), dtype=capi.RECORD_DTYPE)
    for r, (_, s, sh) in enumerate(reads):
        a, b = int(off[r]), int(off[r + 1])
        rec["read"][a:b] = r; rec["sketch"][a:b] = s; rec["shared"][a:b] = sh
    rec["ref_contig"] = np.arange(len(rec)) if contig_of is None else [contig_of(i) for i in range(len(rec))]
    rec["ref_start"] = 100
    return np.array([L for L, _, _ in reads], dtype=np.int32), off, rec


def device_qualities(ctx, reads):
    from metamaps_amd import capi
    rl, off, rec = records(reads)
    M = capi.Mapping.from_parts(ctx, rl, [(off, rec)], [0], K, 8)
    M.add_qualities(K)
    off2, got = M.fetch()
    M.close()
    assert np.array_equal(off2, off) and np.array_equal(got["shared"], rec["shared"]) and np.array_equal(got["read"], rec["read"])
    return off, got["mapq"].astype(np.float64)


def exact_qualities(L, s, shared):
    """(exact normalised qualities as mpf, the bound on a device quality's relative error) of one read"""
    p = post_ref.success_p(max(post_ref.identity(x, s, K) for x in shared), L, K)
    mass = [post_ref.pmf_exact(s, p, x) for x in shared]
    S = [post_ref.pmf_scale(s, p, x) for x in shared]
    total = mpmath.fsum(mass)
    s_sum = float(mpmath.fsum(m * t for m, t in zip(mass, S)) / total)          # the sum errs as its terms do, each by its weight in it
    # a mass errs by PMF_C_DEVICE * S ulps (post_ref), the sum by the same constant times its weighted S plus half an ulp per addition in record
    # order, the division by half an ulp: for the record that dominates the sum this is twice the bound of a mass
    bound = [post_ref.PMF_C_DEVICE * (t + s_sum) * post_ref.ULP + (len(shared) + 1) * 2.0 ** -53 for t in S]
    return [m / total for m in mass], bound, p


def k8_ladder():
    """1, 2, 255, 256, 257 and 1 025 records, reads without records before, between and after, three reads inside one 256-record block
    (records 1 796 .. 1 945 of block 7), every sketch size of the host test, shared 0, 1, s - 1"""
    rng = np.random.default_rng(801)
    cl = lambda n, lo, hi, extra: [int(x) for x in rng.permutation(np.concatenate([rng.integers(lo, hi + 1, n - len(extra)), extra]))]
    return [(1_000, 250, []),
            (1_000, 17, [5]),
            (1_000, 2, [1, 0]),
            (10_000, 2_222, []),
            (1_125, 250, cl(255, 150, 200, [0, 1])),
            (10_000, 2_222, cl(256, 1_500, 1_650, [0, 1])),
            (54_000, 12_000, cl(257, 9_000, 9_300, [0, 1])),
            (1_000, 1, []),
            (270_000, 60_000, cl(1_025, 45_000, 45_600, [0, 1])),
            (1_000, 17, []),
            (147_456, 32_768, cl(100, 20_000, 20_300, [32_767])),
            (1_000, 1, cl(30, 0, 1, [1])),
            (10_000, 250, cl(20, 100, 140, [249])),
            (1_000, 250, [])]


def test_k8_qualities_against_exact_masses(ctx):
    """normalised qualities against exact binomial masses over their exact sum.  Measured on an MI355X: see post_ref.PMF_C_DEVICE."""
    reads = k8_ladder()
    off, q = device_qualities(ctx, reads)
    assert [int(x) for x in np.diff(off)] == [0, 1, 2, 0, 255, 256, 257, 0, 1_025, 0, 100, 30, 20, 0]
    assert off[10] // 256 == (off[13] - 1) // 256                  # reads 10, 11 and 12 share a block of the per-record kernels
    worst, n_rel = 0.0, 0
    for r, (L, s, shared) in enumerate(reads):
        if not shared:
            continue
        want, bound, _ = exact_qualities(L, s, shared)
        got = q[off[r]:off[r + 1]]
        assert np.all(np.isfinite(got)) and abs(math.fsum(got) - 1) < 1e-12
        for g, w, b, x in zip(got, want, bound, shared):
            if w < mpmath.mpf("1e-290"):                            # the denormal range of exp: absolutely
                assert abs(g - float(w)) <= 1e-300 + float(w) * b, (r, x, g, float(w))
                continue
            rel = float(abs(mpmath.mpf(float(g)) - w) / w)
            n_rel += 1
            worst = max(worst, rel / b)
            assert rel <= b, (r, s, x, g, float(w), rel, b)
    print(f"K8 on the device: worst relative error / bound = {worst:.4f} over {n_rel} qualities above 1e-290")
    assert n_rel > 400


def test_k8_special_cases(ctx):
    reads = [(10_000, 2_222, [1_644, 2_222, 800]),                 # best record has shared == sketch: p = 1, that record exactly 1, the others exactly 0
             (1_000, 250, [0] * 7),                               # all shared == 0 at length 1 000: p = 0, every mass 1, exactly 1 / n
             (10_000, 2_222, [1_644, 1_600]), (10_000, 2_222, [1_600, 1_644]),                      # the same records in another order
             (10_000, 2_222, [1_644, 1_600, 3]), (10_000, 2_222, [3, 1_644, 1_600]), (10_000, 2_222, [1_600, 3, 1_644])]   # (the third mass is 0)
    assert post_ref.success_p(post_ref.identity(2_222, 2_222, K), 10_000, K) == 1.0 and post_ref.success_p(post_ref.identity(0, 250, K), 1_000, K) == 0.0
    assert float(exact_qualities(*reads[4])[0][2]) == 0.0
    off, q = device_qualities(ctx, reads)
    part = [q[off[r]:off[r + 1]].tolist() for r in range(len(reads))]
    assert part[0] == [0.0, 1.0, 0.0]
    assert part[1] == [1.0 / 7.0] * 7
    assert part[2] == part[3][::-1] and 0 < part[2][1] < part[2][0] < 1
    assert sorted(part[4]) == sorted(part[5]) == sorted(part[6]) == sorted(part[2] + [0.0])


WINDOW = (10_000, 2_222, [1_644] + list(range(778, 804)))


def test_window_of_tiny_qualities_does_not_poison_the_em(ctx):
    """A 10 000-base read whose best record has identity 98.99 and 26 records near 96: their normalised qualities lie in (0, 1e-303), where the
    6-digit round trip of em_entries_kernel once scaled by an infinite power of ten and stored NaN."""
    from metamaps_amd import capi
    L, s, shared = WINDOW
    p = post_ref.success_p(max(post_ref.identity(x, s, K) for x in shared), L, K)
    mass = np.array([post_ref.pmf_float64(s, p, x) for x in shared])
    q64 = mass / math.fsum(mass)                                   # a condition on the input, from the float64 restatement of K8
    assert np.count_nonzero((q64[1:] > 0) & (q64[1:] < 1e-303)) >= 20 and np.count_nonzero(q64 > post_ref.DBL_MIN) >= 1
    rl, off, rec = records([WINDOW])
    n = len(rec)
    M = capi.Mapping.from_parts(ctx, rl, [(off, rec)], [0], K, 8)
    M.add_qualities(K)
    _, got = M.fetch()
    e = ctx.em_from_mapping(M, np.arange(n), np.full(n, 50_000), n)               # each record on its own contig, each contig its own taxon
    f = np.full(n, 1.0 / n)
    part, ll = e.iterate(f)
    post, best = e.posteriors(f)
    assert np.all(np.isfinite(part)) and math.isfinite(ll) and np.all(np.isfinite(post))
    mapq = np.array([post_ref.text6(x) for x in got["mapq"]])
    assert np.count_nonzero((mapq > 0) & (mapq < 1e-303)) >= 1                    # the window is reached on the device as well
    want, want_ll = post_ref.posteriors_reference(off, np.arange(n), mapq, np.full(n, 1.0 / (50_000 - L + 1)), f)
    assert np.allclose(post, want, rtol=1e-12, atol=0) and np.allclose(part, want, rtol=1e-12, atol=0) and np.isclose(ll, want_ll, rtol=1e-12, atol=0)
    assert best[0] == 0
    f_run, lls = e.run(f)
    assert np.all(np.isfinite(f_run)) and np.all(np.isfinite(lls)) and abs(f_run.sum() - 1) < 1e-12
    e.close(); M.close()


def test_nloc_of_em_entries(ctx):
    """1 / nLoc (getMappingLocations, fEM.h:322-346) seen through the posteriors: contigs one shorter than, as long as and one longer than the read"""
    from metamaps_amd import capi
    L = 5_000
    contig_len = np.array([L - 1, L - 1, L - 1, L - 1, L + 1, L - 1, L, L + 1, L + 2], dtype=np.int32)
    contig_taxon = np.array([0, 0, 1, 1, 1, 2, 2, 3, 3], dtype=np.int32)
    # read 0 (length L):     taxon 0: all contigs shorter, mapped to both: 2.  taxon 1: one shorter and mapped, one shorter and unmapped, one longer
    #                        (2 places): 3.  taxon 2: two records on the same short contig, counted once, and a contig of exactly L (1 place): 2
    # read 1 (length L + 1): contig 4 is exactly as long (1 place), contig 3 shorter and mapped, contig 2 shorter and unmapped: 2.  taxon 3: 1 + 2 = 3
    rec_contig = [0, 1, 2, 4, 5, 5, 6, 3, 4, 7]
    nloc = [2, 2, 3, 3, 2, 2, 2, 2, 2, 3]
    off = np.array([0, 7, 10], dtype=np.int64)
    rec = np.zeros(10, dtype=capi.RECORD_DTYPE)
    rec["read"] = [0] * 7 + [1] * 3; rec["ref_contig"] = rec_contig; rec["sketch"] = 100; rec["shared"] = 50
    rec["mapq"] = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.5, 0.25, 0.125]          # (their own 6-digit texts)
    M = capi.Mapping.from_parts(ctx, np.array([L, L + 1], dtype=np.int32), [(off, rec)], [0], K, 8)
    e = ctx.em_from_mapping(M, contig_taxon, contig_len, 4)
    f = np.array([0.4, 0.3, 0.2, 0.1])
    taxon = contig_taxon[rec_contig]
    assert np.array_equal(e.taxon_counts(), np.bincount(taxon, minlength=4))
    post, _ = e.posteriors(f)
    want, _ = post_ref.posteriors_reference(off, taxon, rec["mapq"], 1.0 / np.array(nloc, dtype=np.float64), f)
    assert np.allclose(post, want, rtol=1e-12, atol=0)
    wrong, _ = post_ref.posteriors_reference(off, taxon, rec["mapq"], np.ones(10), f)
    assert not np.allclose(post, wrong, rtol=1e-3, atol=0)                       # (the posteriors do depend on nLoc)
    e.close(); M.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# K9: the device-resident loop (em_p1 / p2 / p3) against the float64 host EM
# ----------------------------------------------------------------------------------------------------------------------------------
def default_grid(n_reads, n_entries):
    """em_grid without MM_EM_GRID, and the reads per workgroup of em_p1"""
    want = max(256, -(-max(n_reads, 1) // (EM_RBUF * 5 // 6)), -(-max(n_entries, 1) // (EM_LBUF * 7 // 8)))
    n_wg = max(1, min(want, 1 << 20, max(n_reads, 1)))
    return n_wg, -(-n_reads // n_wg)


def random_entries(rng, sizes, n_taxa, taxa=None):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ne = int(off[-1])
    taxon = (rng.integers(0, n_taxa, ne) if taxa is None else rng.choice(taxa, ne)).astype(np.int32)
    mapq = np.array([post_ref.text6(x) for x in 10.0 ** rng.uniform(-6, 0, ne)])
    inv = 1.0 / rng.integers(1, 4_000_000, ne).astype(np.float64)
    return off, taxon, mapq, inv


def problem_mappings_per_read():
    """One read per workgroup on the default grid (51 reads <= 256): 512 mappings or fewer go the LDS form of P1, more go thread-per-read with
    its second pass; 7 .. 17 walk its 8-mapping chunks and clamped indices.  With MM_EM_GRID=1 every read goes thread-per-read."""
    rng = np.random.default_rng(902)
    sizes = [0, 1, 7, 8, 9, 0, 15, 16, 17, 511, 512, 513, 0, 1_023, 1_025, 2_049, 0] * 3
    return random_entries(rng, sizes, 40) + (40,)


def problem_skewed_reads():
    """10 000 reads, most with 1 .. 6 mappings, every 150th with 600: the default grid gives 256 workgroups of 40 reads, of which those holding a
    heavy read exceed the LDS block (thread-per-read) and the others do not (LDS form): both forms in one launch"""
    rng = np.random.default_rng(903)
    sizes = rng.integers(1, 7, 10_000)
    sizes[75::150] = 600
    sizes[rng.integers(0, 10_000, 300)] = 0
    return random_entries(rng, sizes, 60) + (60,)


TAXON_ENTRIES = [1, 63, 64, 65, 511, 512, 513, 1_024, 1_025, 4_096, 4_097, 4_608]


def problem_entries_per_taxon():
    """P2's 512-entry items and P3's 8-item chunks: taxa with 1 .. 4 608 entries (nine items), a pair of twins (taxa 14 and 15: the same reads, the
    same qualities and 1 / nLoc, 700 entries) and taxa without entries (0, 7, 16)"""
    rng = np.random.default_rng(904)
    n_reads, n_taxa = 5_000, 17
    with_entries = [t for t in range(n_taxa) if t not in (0, 7, 15, 16)]
    counts = dict(zip(with_entries, TAXON_ENTRIES + [700]))        # taxon 15 follows 14 wherever it goes
    assert len(with_entries) == len(TAXON_ENTRIES) + 1
    per_read = [[] for _ in range(n_reads)]
    for t, c in counts.items():
        for r in np.sort(rng.choice(n_reads, c, replace=False)):
            q, w = post_ref.text6(10.0 ** rng.uniform(-6, 0)), 1.0 / int(rng.integers(1, 4_000_000))
            per_read[r].append((t, q, w))
            if t == 14:
                per_read[r].append((15, q, w))
    off = np.concatenate([[0], np.cumsum([len(x) for x in per_read])]).astype(np.int64)
    flat = [e for x in per_read for e in x]
    return off, np.array([e[0] for e in flat], dtype=np.int32), np.array([e[1] for e in flat]), np.array([e[2] for e in flat]), n_taxa


def problem_present_taxa(n_present, n_taxa):
    """P3's 256-taxon stride: n_present taxa with entries among n_taxa"""
    rng = np.random.default_rng(905 + n_present)
    taxa = np.sort(rng.choice(n_taxa, n_present, replace=False))
    sizes = rng.integers(0, 5, 700)
    off, taxon, mapq, inv = random_entries(rng, sizes, n_taxa, taxa)
    taxon[:n_present] = taxa                                        # every present taxon at least once
    return off, taxon, mapq, inv, n_taxa


# The stop rule must not flip on rounding: the margins of the reference's last two iterations, (|gain - 1|, |1 - ll / ll_prev - 1e-4| / 1e-4), as
# measured when these seeds were chosen — the test asserts at least 1e-6 for each before it looks at the device.
LOOP_PROBLEMS = {
    "mappings_per_read": problem_mappings_per_read,                # 9 iterations; (0.90, 0.61), (0.94, 0.016)
    "skewed_reads": problem_skewed_reads,                          # 4; (0.28, 0.94), (0.95, 1.0)
    "entries_per_taxon": problem_entries_per_taxon,                # 5; (8.2, 0.022), (0.23, 0.92)
    "present_1_of_300": lambda: problem_present_taxa(1, 300),      # 3; (3.2e3, 2.4e3), (1, 1)
    "present_255_of_300": lambda: problem_present_taxa(255, 300),  # 5; (0.79, 0.38), (0.37, 0.51)
    "present_256_of_300": lambda: problem_present_taxa(256, 300),  # 5; (1.3, 0.78), (0.21, 0.39)
    "present_257_of_300": lambda: problem_present_taxa(257, 300),  # 5; (0.55, 0.12), (0.46, 0.61)
    "one_taxon": lambda: problem_present_taxa(1, 1),               # 2; (1, 1)
}


def loop_reference(name):
    off, taxon, mapq, inv, n_taxa = LOOP_PROBLEMS[name]()
    f0 = np.full(n_taxa, 1.0 / n_taxa)
    f, lls, margins = post_ref.em_reference(off, taxon, mapq, inv, n_taxa, f0)
    return (off, taxon, mapq, inv, n_taxa, f0), f, lls, margins


@pytest.mark.parametrize("name", list(LOOP_PROBLEMS))
def test_em_loop_against_host_reference(ctx, monkeypatch, name):
    (off, taxon, mapq, inv, n_taxa, f0), f_ref, ll_ref, margins = loop_reference(name)
    assert 2 <= len(ll_ref) < 1000
    for gain_off, rel_off in margins[-2:]:
        assert gain_off >= 1e-6 and rel_off >= 1e-6, margins[-2:]
    sizes = np.diff(off)
    if name == "mappings_per_read":
        n_wg, per_wg = default_grid(len(sizes), len(taxon))
        assert per_wg == 1 and sizes[0] == sizes[-1] == 0 and {511, 512, 513} <= set(sizes.tolist())
    if name == "skewed_reads":
        n_wg, per_wg = default_grid(len(sizes), len(taxon))
        block = np.add.reduceat(sizes, np.arange(0, len(sizes), per_wg))
        assert per_wg <= EM_RBUF and np.count_nonzero(block <= EM_LBUF) > 50 and np.count_nonzero(block > EM_LBUF) > 50
    if name == "entries_per_taxon":
        counts = np.bincount(taxon, minlength=n_taxa)
        assert sorted(counts[counts > 0].tolist()) == sorted(TAXON_ENTRIES + [700, 700]) and -(-4_608 // EM_ITEM) == 9
    for grid in (None, "1"):
        monkeypatch.delenv("MM_EM_GRID", raising=False)
        if grid:
            monkeypatch.setenv("MM_EM_GRID", grid)
        e = ctx.em(off, taxon, mapq, inv, n_taxa)
        f1, _ = e.run(f0, max_iter=1)
        f, lls = e.run(f0)
        e.close()
        assert len(lls) == len(ll_ref), (grid, len(lls), len(ll_ref))
        assert np.allclose(lls, ll_ref, rtol=1e-12, atol=0), grid
        assert np.allclose(f, f_ref, rtol=1e-10, atol=1e-300), grid
        absent = np.bincount(taxon, minlength=n_taxa) == 0
        assert np.all(f1[absent] == 0) and np.all(f[absent] == 0)                                  # exactly 0 from the first iteration
        if name == "entries_per_taxon":
            assert f[14] == f[15] and f1[14] == f1[15] and f[14] > 0                            # the twins, to the bit


# ----------------------------------------------------------------------------------------------------------------------------------
# K9: the per-call kernels (em_estep / em_taxon_sum / em_best) and the empty problem
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads", [255, 256, 257, 65_537])
def test_iterate_and_posteriors(ctx, n_reads):
    rng = np.random.default_rng(1_000 + n_reads)
    sizes = rng.integers(0, 6, n_reads)
    sizes[[0, n_reads - 1]] = [3, 2]
    n_taxa = 50
    off, taxon, mapq, inv = random_entries(rng, sizes, n_taxa)
    f = rng.dirichlet(np.ones(n_taxa))
    twins = np.nonzero(sizes >= 3)[0][::7]                          # reads whose largest likelihood comes twice, bit for bit: entries 1 and 2
    for r in twins:                                                 # (the most frequent taxon at quality 1 and one location; the others at half that or less)
        a, b = int(off[r]), int(off[r + 1])
        inv[a:b] = np.minimum(inv[a:b], 0.5)
        taxon[a + 1:a + 3] = int(np.argmax(f)); mapq[a + 1:a + 3] = 1.0; inv[a + 1:a + 3] = 1.0
    want, want_ll = post_ref.posteriors_reference(off, taxon, mapq, inv, f)
    want_part = np.array([math.fsum(want[taxon == t]) for t in range(n_taxa)])
    e = ctx.em(off, taxon, mapq, inv, n_taxa)
    part, ll = e.iterate(f)
    post, best = e.posteriors(f)
    e.close()
    assert np.allclose(post, want, rtol=1e-12, atol=0) and np.allclose(part, want_part, rtol=1e-12, atol=0) and np.isclose(ll, want_ll, rtol=1e-12, atol=0)
    n_decided = 0
    for r in range(n_reads):
        a, b = int(off[r]), int(off[r + 1])
        if a == b:
            assert best[r] == -1
            continue
        assert a <= best[r] < b
        top = np.sort(want[a:b])[::-1]
        if b - a == 1 or top[0] - top[1] > 1e-9 * top[0]:
            assert best[r] == a + int(np.argmax(want[a:b])), r
            n_decided += 1
    assert n_decided > 0.8 * np.count_nonzero(sizes)
    assert len(twins) > 5
    for r in twins:
        assert best[r] == off[r] + 1 and post[off[r] + 1] == post[off[r] + 2]                  # two identical maxima: the first


@pytest.mark.parametrize("n_reads", [0, 5])
def test_empty_problem(ctx, n_reads):
    """No reads, and reads that are all empty.  No taxon has a mapping, so the loop writes 0 for every taxon (fEM.h:606-615 would divide 0 by 0;
    em_p3 divides for the taxa with mappings only), every log-likelihood is 0, and the stop rule never fires (1 - 0 / 0 is no number): the
    caller's limit ends the run."""
    e = ctx.em(np.zeros(n_reads + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), 3)
    f0 = np.array([0.5, 0.25, 0.25])
    part, ll = e.iterate(f0)
    assert part.tolist() == [0, 0, 0] and ll == 0
    post, best = e.posteriors(f0)
    assert len(post) == 0 and best.tolist() == [-1] * n_reads
    f, lls = e.run(f0, max_iter=4)
    assert f.tolist() == [0, 0, 0] and lls.tolist() == [0, 0, 0, 0]
    e.close()
