"""What the pileup and the VCF share (metamaps_amd/csrc/mm_jobs_dev.hpp: the aligned jobs; mm_keytable.hip: the key tables), held to what their two
definitions say about each other.

SNVs.  A pileup key with a code 0-3 comes from a base of an X run that reads A, C, G or T, and from nothing else (a deleted base has code 5, an insertion 6, an N
4); the VCF counts an SNV (w1 == 0, the same w0) for exactly those bases.  So over the same jobs the pileup's (key, count) pairs with a code 0-3 are the VCF's
triples with a code 0-3.  tests/pileup_ref.py and tests/vcf_ref.py must agree on that on the CPU; mm_pileup_events and mm_vcf_events on the device, and with them.

Key tables.  mm_pileup_merge and mm_vcf_merge at the sizes around the 256-thread blocks of the reduction, with a segment head on either side of a block's edge."""
import numpy as np
import pytest

import pileup_ref
import vcf_cases
import vcf_ref
from test_gpu_pileup import arrays
from vcf_cases import D, EQ, I, X


def snv_world():
    """vcf_cases' built cases, and one job each of: exactly 64 and 65 runs (the tile's edge), an X run of 64 and of 65 bases (LONG_RUN), strand -1, use == 0, dist < 0"""
    contigs, built = vcf_cases.built_world()
    jobs = list(built.values())
    tile = [(1, X), (2, EQ), (1, D), (1, EQ), (1, I), (1, X)] * 11
    jobs.append(vcf_cases.job(contigs, 1, 330, tile[:64]))
    jobs.append(vcf_cases.job(contigs, 0, 310, tile[:65]))
    jobs.append(vcf_cases.job(contigs, 0, 500, [(2, EQ), (64, X), (3, EQ)]))
    jobs.append(vcf_cases.job(contigs, 1, 400, [(2, EQ), (65, X), (3, EQ)]))
    jobs.append(vcf_cases.job(contigs, 0, 500, [(1, X), (5, EQ), (2, X, b"TN"), (1, D), (4, EQ)], strand=-1))
    jobs.append(vcf_cases.job(contigs, 0, 500, [(3, X), (5, EQ)], use=0))
    jobs.append(dict(vcf_cases.job(contigs, 0, 500, [(3, X), (5, EQ)]), d=-1, runs=[], first=-1))
    return contigs, jobs


def snvs_of_pileup(table):
    return {k: c for k, c in table.items() if k & 7 < 4}


def snvs_of_vcf(table):
    assert all(w1 == 0 for (w0, w1) in table if w0 & 7 < 4)       # an SNV has no second word
    return {w0: c for (w0, w1), c in table.items() if w0 & 7 < 4}


@pytest.fixture(scope="module")
def snv_want():
    """the X-only pileup counts of snv_world by pileup_ref: computed once, never changed"""
    contigs, jobs = snv_world()
    want = snvs_of_pileup(pileup_ref.table(jobs))
    assert len(want) > 300 and max(want.values()) >= 3 and {k & 7 for k in want} == {0, 1, 2, 3} and {k >> 35 for k in want} == {0, 1}
    return contigs, jobs, want


def test_the_two_references_agree_on_the_snvs(snv_want):
    contigs, jobs, want = snv_want
    assert snvs_of_vcf(vcf_ref.table(jobs, contigs)) == want
    assert [len(j["runs"]) for j in jobs[-7:-5]] == [64, 65] and [max(w >> 4 for w in j["runs"]) for j in jobs[-5:-3]] == [64, 65]
    assert jobs[-3]["strand"] == -1 and jobs[-2]["use"] == 0 and jobs[-1]["d"] < 0
    for j in jobs[-7:-2]:                                           # each added job that contributes has SNVs of its own to lose
        assert snvs_of_pileup(pileup_ref.table([j])) == snvs_of_vcf(vcf_ref.table([j], contigs)) != {}
    assert pileup_ref.table(jobs[-2:]) == {} == vcf_ref.table(jobs[-2:], contigs)


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_pileup_and_vcf_agree_on_the_snvs_of_the_same_jobs(ctx, snv_want):
    import test_gpu_pileup
    import test_gpu_vcf
    contigs, jobs, want = snv_want
    reads, ref = ctx.seqset([j["read"] for j in jobs]), ctx.seqset(contigs)
    try:
        pile = test_gpu_pileup.as_dict(*ctx.pileup_events(reads, ref, **arrays(jobs)))
        vcf = test_gpu_vcf.as_dict(*ctx.vcf_events(reads, ref, **arrays(jobs)))
    finally:
        reads.close(); ref.close()
    assert snvs_of_pileup(pile) == want
    assert snvs_of_vcf(vcf) == want


EDGE_SIZES = (1, 255, 256, 257, 513)


def shuffled(n, *columns):
    order = np.random.default_rng(197 + n).permutation(n)
    return [np.asarray(c)[order] for c in columns]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_pileup_merge_at_the_block_edges(ctx, n):
    import test_gpu_pileup
    counts = np.arange(n, dtype=np.uint32) % 5 + 1
    same = np.full(n, pileup_ref.key(1, 77, 2), dtype=np.uint64)
    distinct = np.array([pileup_ref.key(i % 2, 3 * i, i % 7) for i in range(n)], dtype=np.uint64)
    for name, keys in (("equal", same), ("distinct", distinct)):
        ks, cs = shuffled(n, keys, counts)
        got = test_gpu_pileup.as_dict(*ctx.pileup_merge(ks, cs))
        assert got == pileup_ref.merged(zip(ks, cs)), name
        assert len(got) == (1 if name == "equal" else n), name


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_vcf_merge_at_the_block_edges(ctx, n):
    import test_gpu_pileup
    import test_gpu_vcf
    counts = np.arange(n, dtype=np.uint32) % 5 + 1
    w0_same = np.full(n, pileup_ref.key(1, 77, 5), dtype=np.uint64)
    distinct0 = np.array([pileup_ref.key(i % 2, 3 * i, 5 + i % 2) for i in range(n)], dtype=np.uint64)
    distinct1 = np.array([1 + i % 3 if i % 2 == 0 else (1 + i % 3) << 48 | i % 4 for i in range(n)], dtype=np.uint64)
    # one run of equal w0 whose w1 changes between the sorted rows 255 | 256 and 256 | 257: a segment head on both sides of the edge of a 256-thread block
    edge1 = np.array([1 if i < 256 else 2 if i == 256 else 3 for i in range(n)], dtype=np.uint64)
    # the same edges with w0 changing there and w1 not
    edge0 = np.array([pileup_ref.key(0, 9 if i < 256 else 10 if i == 256 else 11, 5) for i in range(n)], dtype=np.uint64)
    n_edge_keys = {1: 1, 255: 1, 256: 1, 257: 2, 513: 3}[n]
    cases = (("equal", w0_same, np.full(n, 4, dtype=np.uint64), 1), ("distinct", distinct0, distinct1, n), ("w1_edges", w0_same, edge1, n_edge_keys),
             ("w0_edges", edge0, np.full(n, 4, dtype=np.uint64), n_edge_keys))
    for name, w0, w1, n_keys in cases:
        a, b, cs = shuffled(n, w0, w1, counts)
        got = test_gpu_vcf.as_dict(*ctx.vcf_merge(a, b, cs))
        assert got == vcf_ref.merged(zip(a, b, cs)), name
        assert len(got) == n_keys, name
    # second words that are all zero: the pileup's table of the same first words
    a, cs = shuffled(n, distinct0 if n % 2 else edge0, counts)
    w0, w1, c2 = ctx.vcf_merge(a, np.zeros(n, dtype=np.uint64), cs)
    keys, c1 = ctx.pileup_merge(a, cs)
    assert np.array_equal(w0, keys) and np.array_equal(c2, c1) and not w1.any() and len(w1) == len(w0)
    assert test_gpu_pileup.as_dict(keys, c1) == pileup_ref.merged(zip(a, cs))
