"""mm_pileup_events_q and mm_vcf_events_q (the base-quality floor on the device: metamaps_amd/csrc/mm_pileup.hip, mm_vcf.hip and their _core.hpp) through
capi.py against the plain restatement tests/qual_ref.py: the built jobs of tests/qual_cases.py one by one and in one call, 200 random jobs with reads of 50
to 3 000 bases on two contigs; floor 0, and any floor on reads without qualities, give the tables of the calls without a floor bit for bit; the refusals."""
import numpy as np
import pytest

import pileup_ref
import qual_cases
import qual_ref

pytestmark = pytest.mark.gpu

FLOOR = qual_cases.FLOOR


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def arrays(jobs, idx=None):
    op_off = np.zeros(len(jobs) + 1, dtype=np.int64)
    np.cumsum([len(j["runs"]) for j in jobs], out=op_off[1:])
    return dict(read=list(range(len(jobs))) if idx is None else list(idx), strand=[j["strand"] for j in jobs], contig=[j["c"] for j in jobs], dist=[j["d"] for j in jobs],
                first=[j["first"] for j in jobs], op_off=op_off, ops=np.array([w for j in jobs for w in j["runs"]], dtype=np.uint32), use=[j.get("use", 1) for j in jobs])


def pile(keys, counts):
    assert len(keys) == len(counts) and np.all(keys[1:] > keys[:-1])   # unique and ascending
    return {int(k): int(c) for k, c in zip(keys, counts)}


def vcf(w0, w1, counts):
    keys = list(zip(w0.tolist(), w1.tolist()))
    assert len(keys) == len(counts) and all(a < b for a, b in zip(keys, keys[1:]))
    return {k: int(c) for k, c in zip(keys, counts)}


def sets(ctx, contigs, jobs):
    """(reads with their qualities, the same reads without, the reference)"""
    reads = [j["read"] for j in jobs]
    return ctx.seqset(reads, quals=[j["qual"] for j in jobs], qual_offset=0), ctx.seqset(reads), ctx.seqset(contigs)


@pytest.fixture(scope="module")
def built(ctx):
    contigs, jobs = qual_cases.built_world()
    Q, P, R = sets(ctx, contigs, list(jobs.values()))
    yield contigs, jobs, Q, P, R
    Q.close(); P.close(); R.close()


@pytest.fixture(scope="module")
def rand(ctx):
    contigs, jobs = qual_cases.random_world()
    Q, P, R = sets(ctx, contigs, jobs)
    yield contigs, jobs, Q, P, R
    Q.close(); P.close(); R.close()


def test_built_cases_one_by_one(ctx, built):
    contigs, jobs, Q, P, R = built
    for k, (name, j) in enumerate(jobs.items()):
        for floor in (FLOOR, 93):
            assert pile(*ctx.pileup_events(Q, R, min_base_quality=floor, **arrays([j], [k]))) == qual_ref.table([j], floor), (name, floor)
            assert vcf(*ctx.vcf_events(Q, R, min_base_quality=floor, **arrays([j], [k]))) == qual_ref.vcf_table([j], contigs, floor), (name, floor)
    # what the definition says in words, of the device's own tables
    n = lambda name, floor=FLOOR: sum(pile(*ctx.pileup_events(Q, R, min_base_quality=floor, **arrays([jobs[name]], [list(jobs).index(name)]))).values())
    assert n("x1_eq_floor") == 1 and n("x1_below") == 0 and n("x1_eq_floor", FLOOR + 1) == 0
    assert n("x200_low64") == 199 and n("i200_low199") == 0 and n("i200_high") == 1 and n("d70_left_low") == 0 and n("d70_kept") == 70
    assert n("no_qual", 93) == 6


@pytest.mark.parametrize("floor", [1, FLOOR, 41])
def test_built_cases_in_one_call(ctx, built, floor):
    contigs, jobs, Q, P, R = built
    a = arrays(list(jobs.values()))
    assert pile(*ctx.pileup_events(Q, R, min_base_quality=floor, **a)) == qual_ref.table(jobs.values(), floor)
    assert vcf(*ctx.vcf_events(Q, R, min_base_quality=floor, **a)) == qual_ref.vcf_table(jobs.values(), contigs, floor)


@pytest.mark.parametrize("floor", [FLOOR, 41])
def test_200_random_jobs(ctx, rand, floor):
    contigs, jobs, Q, P, R = rand
    a = arrays(jobs)
    got, want = pile(*ctx.pileup_events(Q, R, min_base_quality=floor, **a)), qual_ref.table(jobs, floor)
    assert got == want
    assert vcf(*ctx.vcf_events(Q, R, min_base_quality=floor, **a)) == qual_ref.vcf_table(jobs, contigs, floor)
    full = pileup_ref.table(jobs)
    assert 0 < len(want) < len(full) and set(want) < set(full)       # a proper, non-empty part of the table without a floor
    if floor == FLOOR:
        dropped = sum(full.values()) - sum(want.values())
        assert 0.2 * sum(full.values()) < dropped < 0.8 * sum(full.values())


@pytest.mark.parametrize("world", ["built", "rand"])
def test_floor_0_and_reads_without_qualities_are_the_calls_without_a_floor(ctx, built, rand, world):
    contigs, jobs, Q, P, R = built if world == "built" else rand
    a = arrays(list(jobs.values()) if world == "built" else jobs)
    pk, pc = ctx.pileup_events(P, R, **a)
    v0, v1, vc = ctx.vcf_events(P, R, **a)
    assert len(pk) > 0 and len(v0) > 0
    for reads, floor in ((Q, 0), (P, 0), (P, 40), (P, 93), (Q, None)):
        k, c = ctx.pileup_events(reads, R, min_base_quality=floor, **a)
        assert np.array_equal(k, pk) and np.array_equal(c, pc), floor
        w0, w1, n = ctx.vcf_events(reads, R, min_base_quality=floor, **a)
        assert np.array_equal(w0, v0) and np.array_equal(w1, v1) and np.array_equal(n, vc), floor


@pytest.mark.parametrize("floor", [-1, 94])
def test_a_floor_out_of_range_is_refused(ctx, built, floor):
    from metamaps_amd import capi
    contigs, jobs, Q, P, R = built
    a = arrays(list(jobs.values()))
    for call, which in ((ctx.pileup_events, "last_pileup_handle"), (ctx.vcf_events, "last_vcf_handle")):
        for reads in (Q, P):
            with pytest.raises(capi.MMError) as e:
                call(reads, R, min_base_quality=floor, **a)
            assert e.value.status == -1 and "min_base_quality" in str(e.value) and getattr(ctx, which) is None
