"""mm_mod_events, mm_mod_merge and mm_mod_finish (modification calls counted on the device: metamaps_amd/csrc/mm_mods.hip, mm_mods_core.hpp) through
capi.py against the plain restatement tests/mods_ref.py: the event cases of tests/mods_cases.py one by one and in one call under the thresholds 0, 204 and
255, a seeded world of 40 jobs on three contigs, jobs that do not contribute and reads without a plane, every rule with its message; merges of 0 and 1
pairs and of unsorted repeated keys; the rows of the finish and its refusals."""
import numpy as np
import pytest

import mods_cases
import mods_ref
import pileup_cases

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
    """the event cases and their sets on the device: made once, never changed"""
    contigs, jobs = mods_cases.event_world()
    reads, ref = ctx.seqset([j["read"] for j in jobs.values()], mods=[j["groups"] for j in jobs.values()]), ctx.seqset(contigs)
    yield contigs, jobs, reads, ref
    reads.close(); ref.close()


def test_the_set_holds_the_planes_of_the_restatement(built):
    _, jobs, reads, _ = built
    for k, j in enumerate(jobs.values()):
        assert reads.fetch_mods(k, len(j["read"])) == (j["plane"] or (bytes(len(j["read"])), bytes(len(j["read"]))))


@pytest.mark.parametrize("T", [0, 204, 255])
def test_event_cases(ctx, built, T):
    contigs, jobs, reads, ref = built
    for k, (name, j) in enumerate(jobs.items()):
        assert as_dict(*ctx.mod_events(reads, ref, min_ml=T, **arrays([j], [k]))) == mods_ref.table([j], T), name
    keys, counts = ctx.mod_events(reads, ref, min_ml=T, **arrays(list(jobs.values())))
    got, want = as_dict(keys, counts), mods_ref.table(jobs.values(), T)
    assert got == want
    assert {mods_ref.unkey(k)[2] for k in want} == {1, -1} and {k & 7 for k in want} >= ({0, 2, 3, 4, 5} if T == 0 else {0, 1, 2, 3, 5}) and (1 in {k & 7 for k in want}) == (T > 0)
    assert all(want[k] == 2 for k in mods_ref.table([jobs["fwd"]], T))  # `same_again`: two jobs on every key of `fwd`
    for name in ("no_eq", "not_used", "not_aligned", "no_plane"):
        assert mods_ref.table([jobs[name]], T) == {}, name
    again = ctx.mod_events(reads, ref, min_ml=T, **arrays(list(jobs.values())))
    assert np.array_equal(again[0], keys) and np.array_equal(again[1], counts)


def test_no_jobs_no_plane_and_jobs_that_do_not_contribute(ctx, built):
    contigs, jobs, reads, ref = built
    keys, counts = ctx.mod_events(reads, ref, **arrays([]))
    assert len(keys) == 0 and len(counts) == 0 and ctx.last_mod_handle not in (None, 0xDEAD)
    some = [jobs[n] for n in ("fwd", "rev", "to_the_end")]
    idx = [list(jobs).index(n) for n in ("fwd", "rev", "to_the_end")]
    assert len(ctx.mod_events(reads, ref, **arrays(some, idx, use=[0, 0, 0]))[0]) == 0
    assert len(ctx.mod_events(reads, ref, **arrays(some, idx, dist=[-1, -1, -1]))[0]) == 0
    assert as_dict(*ctx.mod_events(reads, ref, **arrays(some, idx, use=[0, 1, 0]))) == mods_ref.table([some[1]])
    plain = ctx.seqset([j["read"] for j in some])                   # a set without any plane gives none, and its jobs are still checked
    try:
        assert len(ctx.mod_events(plain, ref, **arrays(some))[0]) == 0
    finally:
        plain.close()


def test_seeded_world(ctx):
    contigs, jobs = mods_cases.random_world()
    want = mods_ref.table(jobs)
    # what the restatement alone gives: every class on both strands, and a position with two listed codes
    assert 35 <= len(jobs) <= 45 and {j["c"] for j in jobs} == {0, 1, 2} and all(100 <= len(j["read"]) <= 3100 for j in jobs)
    assert {(k >> 3 & 1, k & 7) for k in want} == {(s, c) for s in (0, 1) for c in range(6)} and max(want.values()) >= 2
    assert any(k & 7 == 3 and (k & ~7 | 4) in want for k in want)
    reads, ref = ctx.seqset([j["read"] for j in jobs], mods=[j["groups"] for j in jobs]), ctx.seqset(contigs)
    try:
        keys, counts = ctx.mod_events(reads, ref, **arrays(jobs))
        assert as_dict(keys, counts) == want
        half = len(jobs) // 2                                       # two calls and a merge give the table of one call
        a, b = ctx.mod_events(reads, ref, **arrays(jobs[:half], range(half))), ctx.mod_events(reads, ref, **arrays(jobs[half:], range(half, len(jobs))))
        mk, mc = ctx.mod_merge(np.concatenate([b[0], a[0]]), np.concatenate([b[1], a[1]]))
        assert np.array_equal(mk, keys) and np.array_equal(mc, counts)
        rows = ctx.mod_finish(ref, mk, mc, mods_cases.CODE_BASE, 1)
        ref_rows = mods_ref.rows(want, contigs, list(mods_cases.CODE_BASE), 1)
        assert list(zip(*(rows[k].tolist() for k in ("site", "n_mod", "n_canonical", "n_other", "n_fail")))) == [(mods_ref.key(c, p, s, k), a_, b_, o, f) for c, p, s, k, a_, b_, o, f in ref_rows]
        assert {k for _, _, _, k, *_ in ref_rows} == {0, 1, 2} and {s for _, _, s, *_ in ref_rows} == {1, -1}
        two = ctx.mod_finish(ref, mk, mc, mods_cases.CODE_BASE, 2)
        assert len(two["site"]) == len(mods_ref.rows(want, contigs, list(mods_cases.CODE_BASE), 2)) < len(ref_rows)
    finally:
        reads.close(); ref.close()


def test_every_rule(ctx, built):
    from metamaps_amd import capi
    _, jobs, _, _ = built
    contigs, _ = pileup_cases.built_world()
    cases = pileup_cases.broken_jobs(contigs)
    base, good = cases[0][0], jobs["one_base"]
    good = dict(good, c=0)                                          # (its one base lies inside the first contig of this reference too)
    g = [dict(base=b, code=-1, mode=".", skips=[], ml=[]) for b in "ACGT"]   # every base is called canonical
    rs, ref = ctx.seqset([good["read"], base["read"]], mods=[g, g]), ctx.seqset(contigs)
    try:
        assert len(ctx.mod_events(rs, ref, **arrays([good, base]))[0]) > 0
        for j, over, rule in cases:                                 # the second job is the broken one: nothing comes out
            over = dict(over)
            read, contig = [0, over.pop("read", 1)], [good["c"], over.pop("contig", base["c"])]
            a = arrays([good, dict(base, **over)], read, contig=contig)
            with pytest.raises(capi.MMError) as e:
                ctx.mod_events(rs, ref, **a)
            assert e.value.status == -1 and "mm_mod_events: job 1: rule %d:" % rule in str(e.value), (over, rule, str(e.value))
            assert ctx.last_mod_handle is None, (over, rule)
        ok = ctx.mod_events(rs, ref, **arrays([good, dict(base, strand=0, use=0)]))   # a job that is not used is not checked
        assert len(ok[0]) > 0
        for bad in (-1, 256):
            with pytest.raises(capi.MMError) as e:
                ctx.mod_events(rs, ref, min_ml=bad, **arrays([good, base]))
            assert e.value.status == -1 and "min_ml" in str(e.value)
    finally:
        rs.close(); ref.close()
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6]


def test_merge(ctx):
    from metamaps_amd import capi
    K = mods_ref.key
    k, c = ctx.mod_merge([], [])
    assert len(k) == 0 and len(c) == 0
    k, c = ctx.mod_merge([K(3, 7, -1, 2)], [9])
    assert list(k) == [K(3, 7, -1, 2)] and list(c) == [9]
    rng = np.random.default_rng(404)
    pool = [K(int(rng.integers(0, 5)), int(rng.integers(0, 1 << 20)), int(rng.choice([-1, 1])), int(rng.integers(0, 7))) for _ in range(300)]
    pool += [K((1 << 28) - 1, (1 << 32) - 1, -1, 6), K(0, 0, 1, 0)]
    keys = [pool[int(i)] for i in rng.integers(0, len(pool), size=2000)]
    counts = [int(x) for x in rng.integers(1, 50, size=2000)]
    keys += [K(1, 5, 1, 5)] * 3 + [K(2, 5, -1, 5)] * 2
    counts += [65535, 1, 40000, 0xFFFFFFFE, 1]                      # sums that cross 65 535, and one that just fits
    assert as_dict(*ctx.mod_merge(keys, counts)) == mods_ref.merged(zip(keys, counts))
    with pytest.raises(capi.MMError) as e:
        ctx.mod_merge(keys + [K(2, 5, -1, 5)], counts + [1])
    assert e.value.status == -1 and "mm_mod_merge" in str(e.value) and ctx.last_mod_handle is None


@pytest.mark.parametrize("world", mods_cases.row_worlds(), ids=lambda w: w[0])
def test_finish(ctx, world):
    name, contigs, t, code_base, min_cov = world
    ref = ctx.seqset(contigs)
    try:
        keys = sorted(t)
        got = ctx.mod_finish(ref, keys, [t[k] for k in keys], code_base, min_cov)
    finally:
        ref.close()
    want = mods_ref.rows(t, contigs, list(code_base), min_cov)
    assert list(zip(*(got[k].tolist() for k in ("site", "n_mod", "n_canonical", "n_other", "n_fail")))) == [(mods_ref.key(c, p, s, k), a, b, o, f) for c, p, s, k, a, b, o, f in want]
    assert (len(want) > 0) == (name != "nothing")


def test_finish_refusals(ctx):
    from metamaps_amd import capi
    ref = ctx.seqset([b"ACGT" * 7 + b"AC", b"CCAAGT"])
    K = mods_ref.key
    try:
        for keys in ([K(0, 5, 1, 1), K(0, 4, 1, 1)], [K(0, 5, 1, 1), K(0, 5, 1, 1)], [K(0, 30, 1, 1)], [K(2, 0, 1, 1)], [K(0, 5, 1, 6)], [K(0, 5, -1, 7)]):
            with pytest.raises(capi.MMError) as e:
                ctx.mod_finish(ref, keys, [1] * len(keys), "CCA", 1)
            assert e.value.status == -1 and "mm_mod_finish" in str(e.value) and ctx.last_mod_handle is None, keys
        for code_base, cov in (("", 1), ("CCAAC", 1), ("CN", 1), ("C", 0)):
            with pytest.raises(capi.MMError) as e:
                ctx.mod_finish(ref, [K(0, 5, 1, 0)], [1], code_base, cov)
            assert e.value.status == -1 and "mm_mod_finish" in str(e.value), (code_base, cov)
    finally:
        ref.close()
