"""Every size-class edge of the per-read kernels against the oracle, bit for bit.

The per-read kernels are picked at run time from the size of a read's work; each pick has hard edges, and the reads here sit on both sides
of every one of them.  They are made by tests/size_ladder.py (exact counts by the oracle, duplicate-rich sequence), and every test first
asserts from the device's own offsets that each read has exactly the planned count: a ladder that drifts off its edge fails.

  K1  tiles of 2 048 k-mer positions, cut per sequence (a tile never spans two reads); from 1 025 minimizers in a tile the staging
      overflows, which raises one flag for the whole batch and sends all of it to the two-pass scheme: so each length runs alone, where
      only its own tiles decide, and all run as neighbours of one batch, which the 1 025 of one read then takes to the two-pass scheme.
      Position counts 1 023 .. 1 025, 2 047 .. 2 049, 4 095 .. 4 097 at k in {15, 16}, w in {1, 2, 8}; at k = 15, w = 1 every position is a
      minimizer (an odd k has no k-mer equal to its reverse complement), so 1 023 / 1 024 / 1 025 positions are as many minimizers in the
      first tile.
  K2  sketch_radix_kernel<IPT>, IPT of size_ladder.K2_IPTS, the smallest with 256 * IPT >= minimizers; from 16 385 on sketch_keys_kernel + segmented
      sort + sketch_finish_kernel.  Minimizer counts E - 1, E, E + 1 for every E = 256 * IPT, and 0, 1, 2, 255, 256, 257, 16 386
      (k = 16, w = 2: 16 386 minimizers are a read of ~25 kb).
  K3  the fused streaming kernel up to SF_SMAX = 2 816 sketch hashes, the two-pass kernels beyond: sketch sizes 2 815, 2 816, 2 817.
  K4  sort_hits_radix_kernel<IPT>, IPT of size_ladder.K4_IPTS; zero or one hit is not sorted; from 4 097 hits on the segmented sort.  Raw hit counts
      E - 1, E, E + 1 for every E = 256 * IPT, and 0, 1, 2, 4 098 (k = 16, w = 2: 4 098 hits are a read of ~6 kb).
  K5  by sketch size s (mm_map.hip l2_host_groups, mm_l1.hpp l2_group_kernel, mm_l2.hpp):
        A  s <= 3 072    four / two candidates per workgroup, 16-bit code words
        B  s <= 7 168    four-wave workgroups, masks in global memory
        D  s <= 16 384   as B, launched on its own
        C  s <  32 768   one wave per workgroup, 16-bit counters                     (edges 3 072 | 3 073, 7 168 | 7 169, 16 384 | 16 385)
        dense path from MM_L2_DENSE_FROM (default 13 000: 12 999 | 13 000) — so D ends at 12 999 and C is empty unless the switch is raised
        L2_SKETCH_LIMIT = 32 768: from there every candidate is dense and the sketch is searched through the bucket table (32 767 | 32 768)
      (k = 16, w = 1: a sketch of 32 769 hashes is a read of ~39 kb).

Results are integers and compared exactly; the one exception is the existing rule for candidates the identity filter rejects, whose
`shared` may stop below the oracle's maximum."""
import numpy as np
import pytest

import size_ladder as sl

pytestmark = pytest.mark.gpu

class World:
    """device index + oracle index of world_contigs, and the oracle's answer per read, computed once and shared"""

    def __init__(self, ctx, oracle, tmpdir, k, w, source_seed):
        self.ctx, self.oracle, self.k, self.w = ctx, oracle, k, w
        self.contigs = sl.world_contigs(source_seed)
        fasta = str(tmpdir / f"world_{k}_{w}.fa")
        sl.write_fasta(fasta, self.contigs)
        self.S = ctx.seqset(self.contigs)
        self.idx = ctx.index(self.S, k, w)
        self.oi = oracle.index(fasta, k, w)
        assert self.idx.freq_threshold == self.oi.freq_threshold
        self._expected = {}

    def expected(self, q):
        if q not in self._expected:
            self._expected[q] = self.oi.map_read(q, 80.0) if len(q) >= max(self.k, self.w) else None
        return self._expected[q]

    def close(self):
        self.oi.close(); self.idx.close(); self.S.close()


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world_w2(ctx, oracle_lib, tmp_path_factory):
    wd = World(ctx, oracle_lib, tmp_path_factory.mktemp("w2"), *sl.K4_KW, source_seed=sl.K2_SEED)
    yield wd
    wd.close()


@pytest.fixture(scope="module")
def world_w1(ctx, oracle_lib, tmp_path_factory):
    wd = World(ctx, oracle_lib, tmp_path_factory.mktemp("w1"), *sl.L2_KW, source_seed=sl.L2_SEED)
    yield wd
    wd.close()


@pytest.fixture(scope="module")
def l2_reads(oracle_lib, world_w1):
    """sketch size -> read, for every size of the K3 and K5 tests: prefixes of the source inside contig SRC_CONTIG of world_w1"""
    sizes = sorted(set(sl.K3_SIZES + sl.K5_SIZES + sl.K5_SMALL_SIZES))
    reads = sl.reads_with_sketch_size(oracle_lib, *sl.L2_KW, sizes, sl.L2_SEED)
    src = world_w1.contigs[sl.SRC_CONTIG][sl.FLANK:-sl.FLANK]
    assert all(src.startswith(q) for q in reads)
    return dict(zip(sizes, reads))


def check_mapping(wd, M, reads, hits):
    """the asserts of test_mapping_stages_match_oracle for every read of the batch: sketch hashes, the raw hit list in sorted order (where the
    batch ran without the pre-filter), candidates, L2 results (accepted: every field; rejected: shared <= the oracle's), records"""
    sk_off, sk_h, _ = M.debug_sketch()
    hit_off, hit_c, hit_w = M.debug_hits()
    cand_off, cand = M.debug_candidates()
    l2 = M.debug_l2(len(cand))
    mh = M.debug_min_hits()
    rec_off, rec = M.fetch()
    n_mapped = n_raw = 0
    n_cand, n_rejected = [0] * len(reads), [0] * len(reads)
    for r, q in enumerate(reads):
        o = wd.expected(q)
        if o is None or len(o["sketch_hash"]) == 0:                 # shorter than k or w, or no minimizer at all: nothing anywhere
            assert sk_off[r + 1] == sk_off[r] and hit_off[r + 1] == hit_off[r] and cand_off[r + 1] == cand_off[r] and rec_off[r + 1] == rec_off[r], r
            continue
        a, b = int(sk_off[r]), int(sk_off[r + 1])
        assert np.array_equal(sk_h[a:b], o["sketch_hash"]), r
        assert mh[r] == o["min_hits"], r
        if hits:
            a, b = int(hit_off[r]), int(hit_off[r + 1])
            assert np.array_equal(hit_c[a:b], o["hit_contig"]) and np.array_equal(hit_w[a:b], o["hit_wpos"]), r
        a, b = int(cand_off[r]), int(cand_off[r + 1])
        assert np.array_equal(cand[a:b], o["cand"]), r
        got, exp = l2[a:b], o["l2"]
        assert np.array_equal(got[:, 0], exp[:, 0]), r
        ok = got[:, 5] == 1
        assert np.array_equal(got[ok][:, [1, 2, 3, 4]], exp[ok][:, [1, 2, 3, 4]]), r
        assert np.all(got[~ok][:, 2] <= exp[~ok][:, 2]), r
        assert int(ok.sum()) == len(o["map"]), r
        n_cand[r], n_rejected[r] = b - a, int((got[:, 5] == 0).sum())
        m = o["map"]
        rr = rec[int(rec_off[r]):int(rec_off[r + 1])]
        assert len(rr) == len(m), r
        assert np.array_equal(rr["ref_contig"], m[:, 0]) and np.array_equal(rr["ref_start"], m[:, 1]), r
        assert np.array_equal(rr["shared"], m[:, 3]) and np.array_equal(rr["sketch"], m[:, 4]) and np.array_equal(rr["strand"], m[:, 5]), r
        n_mapped += len(m) > 0
        n_raw += len(o["hit_contig"])
    st = M.stats()
    assert st["sum_hits"] == n_raw                                  # raw seed hits of the batch, with or without the pre-filter: no look-up is lost
    assert st["n_reads_mapped"] == n_mapped
    return {"n_mapped": n_mapped, "n_cand": n_cand, "n_rejected": n_rejected, "records": (rec_off, rec)}


def check_candidates_matter(sizes, res):
    """the K3 and K5 batches are no single-candidate runs: every read has its source and the diverged copies as candidates (so the groups of
    four and of two candidates per workgroup fill), and L2 rejects at least one candidate of every read at an edge (the `shared <=` rule has
    cases on both sides of each)"""
    assert res["n_mapped"] == len(sizes)
    assert all(c >= 3 for c in res["n_cand"]), res["n_cand"]
    assert all(n >= 1 for s, n in zip(sizes, res["n_rejected"]) if s not in sl.K3_FAR), res["n_rejected"]


# ---- K1

@pytest.mark.parametrize("k,w", sl.K1_KW)
def test_k1_tile_edges(ctx, oracle_lib, k, w):
    """reads that end one position before, on and one behind a tile border (and the staging overflow at 1 025 minimizers of a tile).  Tiles are
    cut per read, and one overflowing tile sends its whole batch to the two-pass scheme: each read alone isolates 1 024 from 1 025, and all as
    neighbours of one batch go through the tile look-up of several sequences (and, at k = 15, w = 1, through the two-pass scheme together)"""
    src = sl.source_sequence(47 + k + w, 60_000)
    seqs = [src[i * 5003:i * 5003 + p + k - 1] for i, p in enumerate(sl.K1_POSITIONS)]
    exp = [oracle_lib.minimizers(q, k, w) for q in seqs]
    if (k, w) == (15, 1):
        assert [len(e[0]) for e in exp] == sl.K1_POSITIONS         # every position a minimizer: 1 023, 1 024, 1 025 in the first tile

    def check(batch, which):
        S = ctx.seqset(batch)
        off, h, wp, st = ctx.minimizers(S, k, w)
        S.close()
        for j, i in enumerate(which):
            a, b = int(off[j]), int(off[j + 1])
            assert b - a == len(exp[i][0]), (k, w, sl.K1_POSITIONS[i], len(which))
            assert np.array_equal(h[a:b], exp[i][0]) and np.array_equal(wp[a:b], exp[i][1]) and np.array_equal(st[a:b], exp[i][2]), (k, w, sl.K1_POSITIONS[i], len(which))

    for i in range(len(seqs)):
        check([seqs[i]], [i])
    check(seqs, list(range(len(seqs))))
    order = sl.shuffled(len(seqs), 3).tolist()
    check([seqs[i] for i in order], order)


# ---- K2

@pytest.fixture(scope="module")
def k2_ladder(oracle_lib):
    """the K2 reads in shuffled order, and per read: count, the sketch by a stable sort (hashes, strand of the first of every run, run has one
    strand only), the oracle's own sketch (std::sort + std::unique on the same minimizers)"""
    k, w = sl.K2_KW
    order = sl.shuffled(len(sl.K2_COUNTS), 11)
    counts = [sl.K2_COUNTS[i] for i in order]
    reads = sl.reads_with_minimizers(oracle_lib, k, w, counts, sl.K2_SEED)
    fasta_seq = sl.random_contig(107, 3000)
    per_read = []
    for q in reads:
        h, _, st = oracle_lib.minimizers(q, k, w)
        per_read.append(sl.sketch_of(h, st))
    return {"counts": counts, "reads": reads, "sketch": per_read, "tiny": fasta_seq}


@pytest.fixture(scope="module")
def tiny_world(ctx, oracle_lib, k2_ladder, tmp_path_factory):
    k, w = sl.K2_KW
    fasta = str(tmp_path_factory.mktemp("tiny") / "tiny.fa")
    sl.write_fasta(fasta, [k2_ladder["tiny"]])
    S = ctx.seqset([k2_ladder["tiny"]])
    idx = ctx.index(S, k, w)
    oi = oracle_lib.index(fasta, k, w)
    oracle_sketch = []
    for q in k2_ladder["reads"]:
        o = oi.map_read(q, 80.0) if len(q) >= max(k, w) else None
        oracle_sketch.append((o["sketch_hash"], o["sketch_strand"]) if o else (np.zeros(0, np.uint32), np.zeros(0, np.int32)))
    yield {"idx": idx, "oracle_sketch": oracle_sketch}
    oi.close(); idx.close(); S.close()


def check_k2(ctx, idx, lad, oracle_sketch, which, eager):
    """one batch of the reads `which` of the ladder through sketch_batch (K1 + K2 alone; it stops in front of the strand tie-break) and through
    map_batch against a tiny index (which resolves the strands of mixed runs in eager mode and counts the ambiguous reads)"""
    k, w = sl.K2_KW
    reads = [lad["reads"][i] for i in which]
    R = ctx.seqset(reads)
    mz_off = ctx.minimizers(R, k, w)[0]
    assert np.diff(mz_off).tolist() == [lad["counts"][i] for i in which]          # the ladder is on its edges
    Sk = ctx.sketch_batch(R, k, w, min_read_len=0)
    M = ctx.map_batch(idx, R, k, w, min_read_len=0)
    n_mixed = 0
    for name, X in (("sketch_batch", Sk), ("map_batch", M)):
        off, h, s = X.debug_sketch()
        for j, i in enumerate(which):
            eh, es, pure = lad["sketch"][i]
            a, b = int(off[j]), int(off[j + 1])
            assert b - a == len(eh), (name, lad["counts"][i])
            assert np.array_equal(h[a:b], eh), (name, lad["counts"][i])
            assert np.array_equal(s[a:b][pure], es[pure]), (name, lad["counts"][i])
            if eager and name == "map_batch":                       # every strand resolved: the oracle's sketch, entry by entry
                oh, os_ = oracle_sketch[i]
                assert np.array_equal(h[a:b], oh) and np.array_equal(s[a:b], os_), lad["counts"][i]
    for i in which:
        n_mixed += not lad["sketch"][i][2].all()
    assert M.stats()["n_ambiguous_sketch_reads"] == n_mixed
    Sk.close(); M.close(); R.close()
    return n_mixed


@pytest.mark.parametrize("eager", [True, False])
def test_k2_ladder_one_batch(ctx, k2_ladder, tiny_world, monkeypatch, eager):
    """every K2 class edge in one shuffled batch, so that the binning forms every run of reads"""
    if eager:
        monkeypatch.setenv("MM_EAGER_TIEBREAK", "1")
    n_mixed = check_k2(ctx, tiny_world["idx"], k2_ladder, tiny_world["oracle_sketch"], list(range(len(k2_ladder["reads"]))), eager)
    assert n_mixed >= 10                                            # the mixed-strand runs are there, in reads on both sides of 16 384


@pytest.mark.parametrize("eager", [True, False])
@pytest.mark.parametrize("count", sl.K2_ALONE)
def test_k2_last_class_edge_alone(ctx, k2_ladder, tiny_world, monkeypatch, eager, count):
    """16 383, 16 384 (the 16-bit payload's last index, the full last class) and 16 385 minimizers (the segmented sort) as single-read batches"""
    if eager:
        monkeypatch.setenv("MM_EAGER_TIEBREAK", "1")
    assert check_k2(ctx, tiny_world["idx"], k2_ladder, tiny_world["oracle_sketch"], [k2_ladder["counts"].index(count)], eager) == 1


# ---- K4

@pytest.fixture(scope="module")
def k4_ladder(world_w2):
    order = sl.shuffled(len(sl.K4_COUNTS), 13)
    counts = [sl.K4_COUNTS[i] for i in order]
    reads = sl.reads_with_hits(world_w2.oi, sl.k4_stretch(world_w2.contigs), *sl.K4_KW, counts, 80.0)
    # the ladder's read of no hit is shorter than k and never active; a random read is: it has a sketch, passes K1 to K3 and comes to the
    # binning of K4 with a count of 0
    stranger = sl.random_contig(111, 600)
    o = world_w2.expected(stranger)
    assert len(o["sketch_hash"]) > 300 and len(o["hit_contig"]) == 0
    at = len(reads) // 2
    reads.insert(at, stranger); counts.insert(at, 0)
    # from 255 hits on a read covers the stretch that contig K4_COPY_CONTIG holds too: the contig bits of the sort key are not constant
    for c, q in zip(counts, reads):
        if c >= 255:
            assert set(world_w2.expected(q)["hit_contig"].tolist()) == {sl.K4_CONTIG, sl.K4_COPY_CONTIG}, c
    return {"counts": counts, "reads": reads, "n_mapped": sum(c >= 1 for c in counts)}     # an exact piece of the reference maps from one hit on


def test_k4_ladder_raw_hits(ctx, world_w2, k4_ladder, monkeypatch):
    """every K4 class edge in one shuffled batch, without the pre-filter: the sort reads the raw hit lists"""
    monkeypatch.setenv("MM_NO_HIT_FILTER", "1")
    R = ctx.seqset(k4_ladder["reads"])
    M = ctx.map_batch(world_w2.idx, R, *sl.K4_KW, min_read_len=0)
    assert np.diff(M.debug_hits()[0]).tolist() == k4_ladder["counts"]
    assert check_mapping(world_w2, M, k4_ladder["reads"], hits=True)["n_mapped"] == k4_ladder["n_mapped"]
    M.close(); R.close()


def test_k4_ladder_filtered_hits(ctx, world_w2, k4_ladder):
    """the same batch under the default switches: the sort reads the staged survivors of the pre-filter"""
    R = ctx.seqset(k4_ladder["reads"])
    M = ctx.map_batch(world_w2.idx, R, *sl.K4_KW, min_read_len=0)
    assert np.diff(M.debug_sketch()[0]).tolist() == [len(o["sketch_hash"]) if o else 0 for o in map(world_w2.expected, k4_ladder["reads"])]
    assert check_mapping(world_w2, M, k4_ladder["reads"], hits=False)["n_mapped"] == k4_ladder["n_mapped"]
    M.close(); R.close()


# ---- K3

def test_k3_fused_to_two_pass_hand_over(ctx, world_w1, l2_reads, monkeypatch):
    """sketches of 2 815, 2 816 (the fused kernel's last) and 2 817 hashes (the two-pass kernels' first) in one batch with reads far from the edge"""
    order = sl.shuffled(len(sl.K3_SIZES), 17)
    sizes = [sl.K3_SIZES[i] for i in order]
    reads = [l2_reads[s] for s in sizes]
    R = ctx.seqset(reads)
    M = ctx.map_batch(world_w1.idx, R, *sl.L2_KW, min_read_len=0)
    assert np.diff(M.debug_sketch()[0]).tolist() == sizes
    res = check_mapping(world_w1, M, reads, hits=False)
    check_candidates_matter(sizes, res)
    off, rec = res["records"]
    monkeypatch.setenv("MM_NO_HIT_FILTER", "1")
    M2 = ctx.map_batch(world_w1.idx, R, *sl.L2_KW, min_read_len=0)
    off2, rec2 = M2.fetch()
    assert np.array_equal(off, off2) and rec.tobytes() == rec2.tobytes()
    M.close(); M2.close(); R.close()


# ---- K5

def run_k5(ctx, wd, l2_reads, sizes, seed):
    order = sl.shuffled(len(sizes), seed)
    sizes = [sizes[i] for i in order]
    reads = [l2_reads[s] for s in sizes]
    R = ctx.seqset(reads)
    M = ctx.map_batch(wd.idx, R, *sl.L2_KW, min_read_len=0)
    assert np.diff(M.debug_sketch()[0]).tolist() == sizes
    check_candidates_matter(sizes, check_mapping(wd, M, reads, hits=False))
    assert M.stats()["n_reads_giant"] == sum(s >= sl.L2_SKETCH_LIMIT for s in sizes)
    M.close(); R.close()


def test_k5_class_edges_default_switches(ctx, world_w1, l2_reads):
    """A | B at 3 072, B | D at 7 168, D | dense at 13 000, 16 384 inside the dense path, dense | giant at 32 768, in one batch"""
    run_k5(ctx, world_w1, l2_reads, sl.K5_SIZES, 19)


def test_k5_dense_hand_over_at_a_small_size(ctx, world_w1, l2_reads, monkeypatch):
    """MM_L2_DENSE_FROM = 1 500: the hand-over to the dense path inside class A, with one read that stays far above it"""
    monkeypatch.setenv("MM_L2_DENSE_FROM", str(sl.K5_SMALL_DENSE_FROM))
    run_k5(ctx, world_w1, l2_reads, sl.K5_SMALL_SIZES + [3073], 23)


def test_k5_lds_classes_up_to_the_sketch_limit(ctx, world_w1, l2_reads, monkeypatch):
    """MM_L2_DENSE_FROM beyond every read: 13 000 and 16 384 stay in class D, 16 385 .. 32 767 take the one-wave class C, 32 768 is dense all the same"""
    monkeypatch.setenv("MM_L2_DENSE_FROM", str(2 * sl.L2_SKETCH_LIMIT))
    run_k5(ctx, world_w1, l2_reads, sl.K5_LDS_SIZES, 29)
