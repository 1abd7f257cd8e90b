"""mm_errprof_events and mm_errprof_finish (the error profile walked on the device: metamaps_amd/csrc/mm_errprof.hip, mm_errprof_core.hpp) through capi.py
against the plain restatement tests/errprof_ref.py: the built cases of tests/errprof_cases.py one by one and in one call (on a set that mixes reads with and
without qualities and on one without a plane), 200 random jobs with the conservation laws, 0 jobs and jobs that do not contribute, every refusal, MM_ERRPROF_GROUPS
at 1 and 3 with G - 1, G and G + 1 jobs; the ranks, equal keys, orders, skipped keys and the refusal of the finish."""
import os

import numpy as np
import pytest

import errprof_cases
import errprof_ref
from test_gpu_pileup import arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def sets(ctx, contigs, jobs, plane=True):
    quals = [bytes(j["qual"]) if j.get("qual") else None for j in jobs] if plane else None
    return ctx.seqset([j["read"] for j in jobs], quals=quals, qual_offset=0), ctx.seqset(contigs)


def as_lists(got):
    counters, cols, keys = got
    return [int(v) for v in counters], [[int(v) for v in c] for c in cols], [int(k) for k in keys]


@pytest.fixture(scope="module")
def built(ctx):
    """the built cases and their sets on the device: made once, never changed"""
    contigs, jobs = errprof_cases.built_world()
    reads, ref = sets(ctx, contigs, list(jobs.values()))
    yield contigs, jobs, reads, ref
    reads.close(); ref.close()


def test_built_cases_one_by_one(ctx, built):
    contigs, jobs, reads, ref = built
    for k, (name, j) in enumerate(jobs.items()):
        assert as_lists(ctx.errprof_events(reads, ref, **arrays([j], [k]))) == errprof_ref.profile([j], contigs), name


def test_built_cases_in_one_call(ctx, built):
    contigs, jobs, reads, ref = built
    all_jobs = list(jobs.values())
    got = as_lists(ctx.errprof_events(reads, ref, **arrays(all_jobs)))
    assert got == errprof_ref.profile(all_jobs, contigs)
    assert as_lists(ctx.errprof_events(reads, ref, **arrays(all_jobs))) == got


def test_a_set_without_a_plane(ctx, built):
    contigs, jobs, _, ref = built
    bare = [dict(j, qual=None) for j in jobs.values()]
    reads, ref2 = sets(ctx, contigs, bare, plane=False)
    try:
        got = as_lists(ctx.errprof_events(reads, ref2, **arrays(bare)))
    finally:
        reads.close(); ref2.close()
    assert got == errprof_ref.profile(bare, contigs)
    t = errprof_ref.unflat(got[0])
    assert all(sum(t["qual"][s][:94]) == 0 and t["qual"][s][94] > 0 for s in range(3))


def test_no_jobs_and_jobs_that_do_not_contribute(ctx, built):
    contigs, jobs, reads, ref = built
    assert as_lists(ctx.errprof_events(reads, ref, **arrays([]))) == ([0] * 566, [], [])
    names = ("x65_f", "d65_r", "i65_in_g_r")
    some, idx = [jobs[n] for n in names], [list(jobs).index(n) for n in names]
    nothing = ([0] * 566, [[0] * 6] * 3, [errprof_ref.NO_KEY] * 3)
    assert as_lists(ctx.errprof_events(reads, ref, **arrays(some, idx, use=[0, 0, 0]))) == nothing
    assert as_lists(ctx.errprof_events(reads, ref, **arrays(some, idx, dist=[-1, -1, -1]))) == nothing
    want = errprof_ref.profile([dict(some[0], use=0), some[1], dict(some[2], d=-1)], contigs)
    assert as_lists(ctx.errprof_events(reads, ref, **arrays(some, idx, use=[0, 1, 1], dist=[3, some[1]["d"], -1]))) == want


@pytest.fixture(scope="module")
def random_world(ctx):
    contigs, jobs = errprof_cases.random_world()
    reads, ref = sets(ctx, contigs, jobs)
    yield contigs, jobs, reads, ref, errprof_ref.profile(jobs, contigs)
    reads.close(); ref.close()


def test_200_random_jobs_and_what_they_conserve(ctx, random_world):
    contigs, jobs, reads, ref, want = random_world
    got = as_lists(ctx.errprof_events(reads, ref, **arrays(jobs)))
    assert got == want
    t, cols = errprof_ref.unflat(got[0]), got[1]
    assert sum(map(sum, t["sub"])) == sum(c[0] + c[1] for c in cols)
    assert sum(t["qual"][0]) == sum(c[0] for c in cols) and sum(t["qual"][1]) == sum(c[1] for c in cols) and sum(t["qual"][2]) == sum(c[3] for c in cols)
    assert sum(map(sum, t["indel"][0])) == sum(c[2] for c in cols) and sum(map(sum, t["indel"][1])) == sum(c[4] for c in cols)
    # on reads that say what the runs say the diagonal holds the = columns: the same jobs with every read byte as the runs made it
    import bam_cases
    import edit_cases
    clean = []
    for j in jobs:
        if j["d"] < 0:
            clean.append(j); continue
        runs = [(int(w) >> 4, int(w) & 15) for w in j["runs"]]
        clean.append(dict(j, read=edit_cases.stored(bam_cases.job(b"e", contigs[j["c"]], j["first"], runs, 1)["read"], j["strand"])))
    creads, cref = sets(ctx, contigs, clean)
    try:
        cgot = as_lists(ctx.errprof_events(creads, cref, **arrays(clean)))
    finally:
        creads.close(); cref.close()
    assert cgot == errprof_ref.profile(clean, contigs)
    ct = errprof_ref.unflat(cgot[0])
    assert sum(ct["sub"][a][a] for a in range(5)) == sum(c[0] for c in cgot[1]) > 5000


@pytest.mark.parametrize("groups", [1, 3])
def test_the_groups_do_not_show(ctx, random_world, groups):
    contigs, jobs, reads, ref, want = random_world
    assert "MM_ERRPROF_GROUPS" not in os.environ
    for n in (groups - 1, groups, groups + 1, 50):
        default = as_lists(ctx.errprof_events(reads, ref, **arrays(jobs[:n], list(range(n)))))
        os.environ["MM_ERRPROF_GROUPS"] = str(groups)
        try:
            got = as_lists(ctx.errprof_events(reads, ref, **arrays(jobs[:n], list(range(n)))))
        finally:
            del os.environ["MM_ERRPROF_GROUPS"]
        assert got == default == errprof_ref.profile(jobs[:n], contigs), (groups, n)


def test_every_rule(ctx, built):
    from metamaps_amd import capi
    contigs, jobs, _, ref = built
    cases = errprof_cases.broken_jobs(contigs)
    base, good = cases[0][0], jobs["x65_f"]
    rs = ctx.seqset([good["read"], base["read"]])
    try:
        ok = as_lists(ctx.errprof_events(rs, ref, **arrays([good, base])))
        assert ok == errprof_ref.profile([dict(good, qual=None), base], contigs)
        for j, over, rule in cases:                                 # the second job is the broken one; behind it a third that breaks rule 2: the lowest is named
            over = dict(over)
            read, contig = [0, over.pop("read", 1), 1], [good["c"], over.pop("contig", base["c"]), base["c"]]
            a = arrays([good, dict(base, **over), dict(base, strand=5)], read, contig=contig)
            with pytest.raises(capi.MMError) as e:
                ctx.errprof_events(rs, ref, **a)
            assert e.value.status == -1 and "mm_errprof_events: job 1: rule %d:" % rule in str(e.value), (over, rule, str(e.value))
        # a job that is not used is not checked; rule 7 (dist against the runs) is not the profile's
        assert as_lists(ctx.errprof_events(rs, ref, **arrays([good, dict(base, strand=0, use=0)])))[0] == errprof_ref.profile([dict(good, qual=None)], contigs)[0]
        assert as_lists(ctx.errprof_events(rs, ref, **arrays([good, dict(base, d=77)]))) == ok
    finally:
        rs.close()
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6]


@pytest.mark.parametrize("world", errprof_cases.finish_worlds(), ids=lambda w: w[0])
def test_finish(ctx, world):
    name, n_contigs, keys, cols = world
    listed, rows, total = errprof_ref.finish(keys, cols)
    contig, stats = ctx.errprof_finish(n_contigs, keys, cols if cols else np.zeros((0, 6), dtype=np.int32))
    assert contig.tolist() == listed and stats.tolist() == rows + [total], name
    assert ctx.last_errprof_handle not in (None, 0xDEAD)
    if name == "nothing" or name == "only_skipped":
        assert listed == [] and total == [0] * 12
    if name == "ranks":
        assert listed == [0, 1, 2, 4, 5, 6, 7, 8, 9] and [r[0] for r in rows] == [1, 2, 3, 4, 5, 4, 9, 64, 65] and total[0] == sum(r[0] for r in rows)
        assert rows[5][7:] == [0, 0, 1_000_000, 1_000_000, 1_000_000] and rows[0][7:] == [rows[0][7]] * 5
    if name == "ranks_shuffled":
        assert (listed, rows, total) == errprof_ref.finish(*errprof_cases.finish_worlds()[2][2:])
    if name == "large_sums":
        assert rows[0][1:7] == [6_000_000_000] * 6


def test_finish_refuses_a_contig_out_of_range(ctx):
    from metamaps_amd import capi
    for n_contigs, keys in ((3, [1 << 32 | 5, 3 << 32 | 7, 9 << 32]), (0, [(1 << 64) - 1, 0]), (1, [(1 << 64) - 1, 1 << 32])):
        with pytest.raises(capi.MMError) as e:
            ctx.errprof_finish(n_contigs, keys, [[1, 0, 0, 0, 0, 0]] * len(keys))
        assert e.value.status == -1 and "mm_errprof_finish: entry 1 " in str(e.value) and ctx.last_errprof_handle is None, (n_contigs, str(e.value))
