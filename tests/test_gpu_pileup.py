"""mm_pileup_events, mm_pileup_merge and mm_pileup_finish (the pileup counted on the device: metamaps_amd/csrc/mm_pileup.hip, mm_pileup_core.hpp) through
capi.py against the plain restatement tests/pileup_ref.py: the built cases of tests/pileup_cases.py one by one and in one call, 200 random jobs, 0 jobs
and jobs that do not contribute, every refusal; merges of 0 and 1 pairs, of unsorted repeated keys, sums across 65 535 and the overflow refusal; the depth,
threshold and coverage edges of the finish and its refusal of a table that is not merged."""
import numpy as np
import pytest

import edit_cases
import pileup_cases
import pileup_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def arrays(jobs, idx=None, **over):
    """the call's arrays for jobs whose reads are the entries idx (default 0, 1, ...) of the read set"""
    op_off = np.zeros(len(jobs) + 1, dtype=np.int64)
    np.cumsum([len(j["runs"]) for j in jobs], out=op_off[1:])
    a = dict(read=list(range(len(jobs))) if idx is None else list(idx), strand=[j["strand"] for j in jobs], contig=[j["c"] for j in jobs], dist=[j["d"] for j in jobs],
             first=[j["first"] for j in jobs], op_off=op_off, ops=np.array([w for j in jobs for w in j["runs"]], dtype=np.uint32), use=[j.get("use", 1) for j in jobs])
    a.update(over)
    return a


def as_dict(keys, counts):
    assert len(keys) == len(counts) and np.all(keys[1:] > keys[:-1])   # unique and ascending
    return {int(k): int(c) for k, c in zip(keys, counts)}


@pytest.fixture(scope="module")
def built(ctx):
    """the built cases and their sets on the device: made once, never changed"""
    contigs, jobs = pileup_cases.built_world()
    reads, ref = ctx.seqset([j["read"] for j in jobs.values()]), ctx.seqset(contigs)
    yield contigs, jobs, reads, ref
    reads.close(); ref.close()


def test_built_cases_one_by_one(ctx, built):
    contigs, jobs, reads, ref = built
    for k, (name, j) in enumerate(jobs.items()):
        got = as_dict(*ctx.pileup_events(reads, ref, **arrays([j], [k])))
        assert got == pileup_ref.table([j]), name
    for name in ("eq_only", "not_used", "not_aligned", "empty_read", "runs0"):
        assert pileup_ref.table([jobs[name]]) == {}, name


def test_built_cases_in_one_call(ctx, built):
    contigs, jobs, reads, ref = built
    keys, counts = ctx.pileup_events(reads, ref, **arrays(list(jobs.values())))
    got, want = as_dict(keys, counts), pileup_ref.table(jobs.values())
    assert got == want
    K = pileup_ref.key
    twice = next(iter(pileup_ref.table([jobs["twice_a"]])))
    assert pileup_ref.unkey(twice)[:2] == (1, 54) and got[twice] == 2   # two jobs on one key
    assert got[K(0, 285, 5)] == 1 and got[K(1, 285, 5)] == 1 and list(keys).index(K(0, 285, 5)) < list(keys).index(K(1, 285, 5))
    assert max(want.values()) >= 2 and {k & 7 for k in want} == {0, 1, 4, 5, 6}   # (the built reads mismatch with A or C; the random jobs bring G and T)
    again = ctx.pileup_events(reads, ref, **arrays(list(jobs.values())))
    assert np.array_equal(again[0], keys) and np.array_equal(again[1], counts)


def test_no_jobs_and_jobs_that_do_not_contribute(ctx, built):
    contigs, jobs, reads, ref = built
    keys, counts = ctx.pileup_events(reads, ref, **arrays([]))
    assert len(keys) == 0 and len(counts) == 0 and ctx.last_pileup_handle not in (None, 0xDEAD)
    some = [jobs[n] for n in ("x_at_0", "d65", "x70_rev_n")]
    idx = [list(jobs).index(n) for n in ("x_at_0", "d65", "x70_rev_n")]
    assert pileup_ref.table(some) != {}
    assert len(ctx.pileup_events(reads, ref, **arrays(some, idx, use=[0, 0, 0]))[0]) == 0
    assert len(ctx.pileup_events(reads, ref, **arrays(some, idx, dist=[-1, -1, -1]))[0]) == 0
    got = as_dict(*ctx.pileup_events(reads, ref, **arrays(some, idx, use=[0, 1, 0])))
    assert got == pileup_ref.table([some[1]])


def test_200_random_jobs_in_one_call(ctx):
    contigs, jobs = pileup_cases.random_world()
    reads, ref = ctx.seqset([j["read"] for j in jobs]), ctx.seqset(contigs)
    try:
        got = as_dict(*ctx.pileup_events(reads, ref, **arrays(jobs)))
    finally:
        reads.close(); ref.close()
    want = pileup_ref.table(jobs)
    assert got == want and len(want) > 1000 and max(want.values()) >= 3 and {k & 7 for k in want} == {0, 1, 2, 3, 4, 5, 6}


def test_every_rule(ctx, built):
    from metamaps_amd import capi
    contigs, jobs, reads, ref = built
    cases = pileup_cases.broken_jobs(contigs)
    base, good = cases[0][0], jobs["x_at_0"]
    rs = ctx.seqset([good["read"], base["read"]])
    try:
        ok = as_dict(*ctx.pileup_events(rs, ref, **arrays([good, base])))
        assert ok == pileup_ref.table([good, base])
        for j, over, rule in cases:                                 # the second job is the broken one: nothing comes out
            over = dict(over)
            read, contig = [0, over.pop("read", 1)], [good["c"], over.pop("contig", base["c"])]
            a = arrays([good, dict(base, **over)], read, contig=contig)
            with pytest.raises(capi.MMError) as e:
                ctx.pileup_events(rs, ref, **a)
            assert e.value.status == -1 and "mm_pileup_events: job 1: rule %d:" % rule in str(e.value), (over, rule, str(e.value))
            assert ctx.last_pileup_handle is None, (over, rule)
        # a job that is not used is not checked; rule 7 (dist against the runs) is not the pileup's
        a = arrays([good, dict(base, strand=0, use=0)])
        assert as_dict(*ctx.pileup_events(rs, ref, **a)) == pileup_ref.table([good])
        assert as_dict(*ctx.pileup_events(rs, ref, **arrays([good, dict(base, d=77)]))) == ok
    finally:
        rs.close()
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6]


def test_merge(ctx):
    from metamaps_amd import capi
    K = pileup_ref.key
    k, c = ctx.pileup_merge([], [])
    assert len(k) == 0 and len(c) == 0
    k, c = ctx.pileup_merge([K(3, 7, 2)], [9])
    assert list(k) == [K(3, 7, 2)] and list(c) == [9]
    rng = np.random.default_rng(93)
    pool = [K(int(rng.integers(0, 5)), int(rng.integers(0, 1 << 20)), int(rng.integers(0, 7))) for _ in range(300)] + [K((1 << 29) - 1, (1 << 32) - 1, 6), K(0, 0, 0)]
    keys = [pool[int(i)] for i in rng.integers(0, len(pool), size=2000)]
    counts = [int(x) for x in rng.integers(1, 50, size=2000)]
    keys += [K(1, 5, 5)] * 3 + [K(2, 5, 5)] * 2
    counts += [65535, 1, 40000, 0xFFFFFFFE, 1]                      # sums that cross 65 535, and one that just fits
    assert as_dict(*ctx.pileup_merge(keys, counts)) == pileup_ref.merged(zip(keys, counts))
    assert pileup_ref.merged(zip(keys, counts))[K(2, 5, 5)] == 0xFFFFFFFF
    with pytest.raises(capi.MMError) as e:
        ctx.pileup_merge(keys + [K(2, 5, 5)], counts + [1])
    assert e.value.status == -1 and "mm_pileup_merge" in str(e.value) and ctx.last_pileup_handle is None


@pytest.fixture(scope="module")
def finish_ref(ctx):
    """contigs of the lengths the finish worlds use, one of them with bytes outside A C G T under its sites"""
    rng = np.random.default_rng(94)
    sets = {}
    for clen in ([100, 50, 120, 7], [30, 6]):
        contigs = [bytearray(edit_cases.dna(rng, n)) for n in clen]
        contigs[0][9] = ord("N"); contigs[0][15] = ord("r"); contigs[-1][2] = ord("N")
        sets[tuple(clen)] = ([bytes(c) for c in contigs], ctx.seqset([bytes(c) for c in contigs]))
    yield sets
    for _, s in sets.values():
        s.close()


@pytest.mark.parametrize("world", pileup_cases.finish_worlds(), ids=lambda w: w[0])
def test_finish(ctx, finish_ref, world):
    name, clen, t, iv, min_count, min_frac = world
    contigs, ref = finish_ref[tuple(clen)]
    sites, cov = pileup_ref.finish(t, iv, clen, min_count, min_frac)
    keys = sorted(t)
    got = ctx.pileup_finish(ref, keys, [t[k] for k in keys], [c for c, _, _ in iv], [a for _, a, _ in iv], [b for _, _, b in iv], min_count, min_frac)
    assert list(zip(got["key"].tolist(), got["count"].tolist(), got["depth"].tolist())) == sites
    assert got["ref_byte"].tobytes() == bytes(contigs[pileup_ref.unkey(k)[0]].upper()[pileup_ref.unkey(k)[1]] for k, _, _ in sites)
    assert list(zip(got["alignments"].tolist(), got["covered"].tolist(), got["sum_depth"].tolist())) == cov
    if name == "edges":
        assert b"N" in got["ref_byte"].tobytes() and cov[0] == (6, 51, 65) and cov[2] == (3, 40, 60)
    if name == "frac_half":
        assert [(n, d) for _, n, d in sites] == [(2, 4), (2, 3)] and b"R" in got["ref_byte"].tobytes()


def test_finish_refuses_a_table_that_is_not_merged(ctx, finish_ref):
    from metamaps_amd import capi
    _, ref = finish_ref[(30, 6)]
    K = pileup_ref.key
    for keys in ([K(0, 5, 1), K(0, 4, 1)], [K(0, 5, 1), K(0, 5, 1)], [K(0, 30, 1)], [K(2, 0, 1)], [K(0, 5, 7)]):
        with pytest.raises(capi.MMError) as e:
            ctx.pileup_finish(ref, keys, [1] * len(keys), [0], [0], [9], 1, 0.0)
        assert e.value.status == -1 and "mm_pileup_finish" in str(e.value) and ctx.last_pileup_handle is None, keys
    with pytest.raises(capi.MMError):
        ctx.pileup_finish(ref, [K(0, 5, 1)], [1], [0], [5], [30], 1, 0.0)   # an interval past its contig's end
