"""mm_vcf_events, mm_vcf_merge and mm_vcf_finish (alleles emitted, left-aligned and counted on the device: metamaps_amd/csrc/mm_vcf.hip, mm_vcf_core.hpp) through
capi.py against the plain restatement tests/vcf_ref.py: the built cases of tests/vcf_cases.py one by one, in one call and in several, random jobs of up to 2 kb
on two low-complexity contigs, calls with and without an indel, 0 jobs and jobs that do not contribute, every refusal; merges of 0 and 1 triples, of shuffled
repeated keys that differ in either word, sums across 65 535 and the overflow refusal; the depth, threshold and window edges of the finish and its refusals."""
import numpy as np
import pytest

import vcf_cases
import vcf_ref
from test_gpu_pileup import arrays

pytestmark = pytest.mark.gpu
K = vcf_ref.key


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def as_dict(w0, w1, counts):
    assert len(w0) == len(w1) == len(counts)
    keys = list(zip(w0.tolist(), w1.tolist()))
    assert keys == sorted(set(keys))                                # unique and ascending by (w0, w1)
    return dict(zip(keys, counts.tolist()))


@pytest.fixture(scope="module")
def built(ctx):
    """the built cases and their sets on the device: made once, never changed"""
    contigs, jobs = vcf_cases.built_world()
    reads, ref = ctx.seqset([j["read"] for j in jobs.values()]), ctx.seqset(contigs)
    yield contigs, jobs, reads, ref
    reads.close(); ref.close()


def test_built_cases_one_by_one(ctx, built):
    contigs, jobs, reads, ref = built
    for k, (name, j) in enumerate(jobs.items()):
        got = as_dict(*ctx.vcf_events(reads, ref, **arrays([j], [k])))
        assert got == vcf_ref.table([j], contigs), name
    for name in ("eq_only_f", "lead_d_r", "trail_i_f", "lead_i_then_d_f", "i_with_n_r", "not_used", "not_aligned", "empty_read"):
        assert vcf_ref.table([jobs[name]], contigs) == {}, name


def test_built_cases_in_one_call_and_in_several(ctx, built):
    contigs, jobs, reads, ref = built
    every = list(jobs.values())
    w0, w1, counts = ctx.vcf_events(reads, ref, **arrays(every))
    got, want = as_dict(w0, w1, counts), vcf_ref.table(every, contigs)
    assert got == want
    hp = vcf_cases.HP12[1]
    assert got[K((0, hp - 1, "D", 1))] >= 2 and vcf_ref.table([jobs["same_del_a"], jobs["same_del_b"]], contigs) == {K((0, hp - 1, "D", 1)): 2}
    assert max(want.values()) >= 2 and {k[0] & 7 for k in want} >= {0, 1, 5, 6}
    assert any(k[0] & 7 == 6 and k[1] == 25 << 48 for k in want) and any(k[0] & 7 == 5 and k[1] == 25 for k in want)
    again = ctx.vcf_events(reads, ref, **arrays(every))
    assert all(np.array_equal(a, b) for a, b in zip(again, (w0, w1, counts)))
    parts = []                                                      # three calls and one merge give the same table
    for lo in range(0, len(every), 30):
        parts.append(ctx.vcf_events(reads, ref, **arrays(every[lo:lo + 30], range(lo, min(lo + 30, len(every))))))
    merged = ctx.vcf_merge(*[np.concatenate([p[i] for p in parts]) for i in range(3)])
    assert all(np.array_equal(a, b) for a, b in zip(merged, (w0, w1, counts)))


def test_calls_without_an_indel_and_with_nothing_but_skipped_events(ctx, built):
    contigs, jobs, reads, ref = built
    names = list(jobs)
    for pick in (["x64_f", "x65_r", "x70_n_f", "x_n_between_r"], ["x_n_between_f"], ["i_with_n_f", "lead_i_f"], ["i_with_n_f", "x_at_0_f"]):
        some, idx = [jobs[n] for n in pick], [names.index(n) for n in pick]
        assert as_dict(*ctx.vcf_events(reads, ref, **arrays(some, idx))) == vcf_ref.table(some, contigs), pick
    assert vcf_ref.table([jobs["i_with_n_f"], jobs["lead_i_f"]], contigs) == {}


def test_no_jobs_and_jobs_that_do_not_contribute(ctx, built):
    contigs, jobs, reads, ref = built
    w0, w1, counts = ctx.vcf_events(reads, ref, **arrays([]))
    assert len(w0) == 0 and len(w1) == 0 and len(counts) == 0 and ctx.last_vcf_handle not in (None, 0xDEAD)
    pick = ("x_at_0_f", "d25_r", "hand_rot_f")
    some, idx = [jobs[n] for n in pick], [list(jobs).index(n) for n in pick]
    assert len(vcf_ref.table(some, contigs)) == 3
    assert len(ctx.vcf_events(reads, ref, **arrays(some, idx, use=[0, 0, 0]))[0]) == 0
    assert len(ctx.vcf_events(reads, ref, **arrays(some, idx, dist=[-1, -1, -1]))[0]) == 0
    assert as_dict(*ctx.vcf_events(reads, ref, **arrays(some, idx, use=[0, 1, 0]))) == vcf_ref.table([some[1]], contigs)


def test_random_jobs_in_one_call(ctx):
    contigs, jobs = vcf_cases.random_world(n=120, seed=195, max_span=2000 // 2)
    extra_contigs, long_jobs = vcf_cases.random_world(n=12, seed=196, max_span=1400)   # reads of up to 2 kb
    assert extra_contigs != contigs
    reads_c, ref_c = [j["read"] for j in jobs], contigs
    reads, ref = ctx.seqset(reads_c), ctx.seqset(ref_c)
    reads2, ref2 = ctx.seqset([j["read"] for j in long_jobs]), ctx.seqset(extra_contigs)
    try:
        got = as_dict(*ctx.vcf_events(reads, ref, **arrays(jobs)))
        got2 = as_dict(*ctx.vcf_events(reads2, ref2, **arrays(long_jobs)))
    finally:
        reads.close(); ref.close(); reads2.close(); ref2.close()
    want = vcf_ref.table(jobs, contigs)
    assert got == want and len(want) > 500 and max(want.values()) >= 2 and {k[0] & 7 for k in want} == {0, 1, 2, 3, 5, 6}
    assert any(k[0] & 7 == 6 and k[1] >> 48 > 24 for k in want) and any(k[0] & 7 == 6 and 0 < k[1] >> 48 <= 24 for k in want)
    assert got2 == vcf_ref.table(long_jobs, extra_contigs) and max(len(j["read"]) for j in long_jobs) > 800


def test_every_rule(ctx, built):
    from metamaps_amd import capi
    contigs, jobs, reads, ref = built
    contigs3 = contigs + [vcf_cases.big_contig()]
    cases = vcf_cases.broken_jobs(contigs3)
    base, big, good = cases[0][0], cases[-1][0], jobs["x_at_0_f"]
    rs, ref3 = ctx.seqset([good["read"], base["read"], big["read"]]), ctx.seqset(contigs3)
    try:
        ok = as_dict(*ctx.vcf_events(rs, ref3, **arrays([good, base])))
        assert ok == vcf_ref.table([good, base], contigs3) and len(ok) == 4
        for j, over, rule in cases:                                 # the second job is the broken one: nothing comes out
            over = dict(over)
            read, contig = [0, over.pop("read", 2 if j is big else 1)], [good["c"], over.pop("contig", j["c"])]
            a = arrays([good, dict(j, **over)], read, contig=contig)
            with pytest.raises(capi.MMError) as e:
                ctx.vcf_events(rs, ref3, **a)
            assert e.value.status == -1 and "mm_vcf_events: job 1: rule %d:" % rule in str(e.value), (over, rule, str(e.value))
            assert ctx.last_vcf_handle is None, (over, rule)
        # the lowest offender is reported; a job that is not used is not checked; rule 7 (dist against the runs) is not ours
        a = arrays([dict(base, strand=0), dict(base, first=-1)], [1, 1])
        with pytest.raises(capi.MMError) as e:
            ctx.vcf_events(rs, ref3, **a)
        assert "job 0: rule 2:" in str(e.value)
        a = arrays([good, dict(base, strand=0, use=0)])
        assert as_dict(*ctx.vcf_events(rs, ref3, **a)) == vcf_ref.table([good], contigs3)
        assert as_dict(*ctx.vcf_events(rs, ref3, **arrays([good, dict(base, d=77)]))) == ok
    finally:
        rs.close(); ref3.close()
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6, 8]


def test_merge(ctx):
    from metamaps_amd import capi
    assert all(len(x) == 0 for x in ctx.vcf_merge([], [], []))
    one = K((3, 7, "I", "GAT"))
    got = ctx.vcf_merge([one[0]], [one[1]], [9])
    assert [x.tolist() for x in got] == [[one[0]], [one[1]], [9]]
    rng = np.random.default_rng(197)
    pool = []
    for _ in range(150):                                           # keys that share w0 and differ in w1, and the other way round
        c, pos = int(rng.integers(0, 5)), int(rng.integers(0, 1 << 20))
        pool += [K((c, pos, "S", "ACGT"[int(rng.integers(0, 4))])), K((c, pos, "D", int(rng.integers(1, 1 << 16)))), K((c, pos, "D", 1)),
                 K((c, pos, "I", "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(1, 25)))))), K((c, pos, "I", "A" * 25)), K((c, pos, "I", "T" * 65535))]
    pool += [((1 << 29) - 1 << 35 | (1 << 32) - 1 << 3 | 6, 65535 << 48), K((0, 0, "S", "A"))]
    pick = rng.integers(0, len(pool), size=3000)
    w0, w1 = [pool[int(i)][0] for i in pick], [pool[int(i)][1] for i in pick]
    counts = [int(x) for x in rng.integers(1, 50, size=3000)]
    a, b = K((1, 5, "D", 3)), K((2, 5, "D", 3))
    w0 += [a[0]] * 3 + [b[0]] * 2; w1 += [a[1]] * 3 + [b[1]] * 2
    counts += [65535, 1, 40000, 0xFFFFFFFE, 1]                      # sums that cross 65 535, and one that just fits
    want = vcf_ref.merged(zip(w0, w1, counts))
    assert as_dict(*ctx.vcf_merge(w0, w1, counts)) == want and want[b] == 0xFFFFFFFF and len(want) < 3005
    only_snv = [(k, n) for k, n in zip(zip(w0, w1), counts) if k[1] == 0]   # every w1 is 0
    assert as_dict(*ctx.vcf_merge([k[0] for k, _ in only_snv], [0] * len(only_snv), [n for _, n in only_snv])) == vcf_ref.merged((k[0], 0, n) for k, n in only_snv)
    with pytest.raises(capi.MMError) as e:
        ctx.vcf_merge(w0 + [b[0]], w1 + [b[1]], counts + [1])
    assert e.value.status == -1 and "mm_vcf_merge" in str(e.value) and ctx.last_vcf_handle is None


@pytest.fixture(scope="module")
def finish_ref(ctx):
    contigs = vcf_cases.finish_worlds()[0][1]
    s = ctx.seqset(contigs)
    yield contigs, s
    s.close()


@pytest.mark.parametrize("world", vcf_cases.finish_worlds(), ids=lambda w: w[0])
def test_finish(ctx, finish_ref, world):
    name, contigs, t, iv, min_count, min_frac = world
    assert contigs == finish_ref[0]
    want = vcf_ref.finish(t, iv, contigs, min_count, min_frac)
    keys = sorted(t)
    got = ctx.vcf_finish(finish_ref[1], [k[0] for k in keys], [k[1] for k in keys], [t[k] for k in keys], [c for c, _, _ in iv], [a for _, a, _ in iv], [b for _, _, b in iv],
                         min_count, min_frac)
    assert list(zip(got["w0"].tolist(), got["w1"].tolist(), got["count"].tolist(), got["depth"].tolist(), [bytes(w) for w in got["window"]])) == want
    if name == "edges":
        assert len(want) == len(t) and any(b"N" in w[4] for w in want) and any(b"R" in w[4] for w in want) and any(w[4][1:] == b"\0" * 24 for w in want)
    if name == "frac_half":
        assert [(n, d) for _, _, n, d, _ in want] == [(2, 4), (2, 4), (2, 3)]
    if name in ("nothing", "intervals_only"):
        assert len(got["w0"]) == 0 and got["window"].shape == (0, 25)


def test_finish_refuses_a_table_that_is_not_merged_or_holds_no_allele(ctx, finish_ref):
    from metamaps_amd import capi
    _, ref = finish_ref
    S, Dl, In = (lambda c, p: K((c, p, "S", "C"))), (lambda c, p, n: K((c, p, "D", n))), (lambda c, p, s: K((c, p, "I", s)))
    bad = ([S(0, 5), S(0, 4)], [S(0, 5), S(0, 5)], [Dl(0, 5, 3), Dl(0, 5, 2)], [S(0, 100)], [S(2, 0)], [(S(0, 5)[0] | 7, 0)], [(S(0, 5)[0] & ~7 | 4, 0)], [(S(0, 5)[0], 1)],
           [Dl(0, 5, 95)], [(Dl(0, 5, 1)[0], 0)], [(Dl(0, 5, 1)[0], 1 << 16)], [(In(0, 5, "A")[0], 0)], [(In(0, 5, "A")[0], 1 << 48 | 4)], [(In(0, 5, "A")[0], 25 << 48 | 1)])
    for keys in bad:
        with pytest.raises(capi.MMError) as e:
            ctx.vcf_finish(ref, [k[0] for k in keys], [k[1] for k in keys], [1] * len(keys), [0], [0], [9], 1, 0.0)
        assert e.value.status == -1 and "mm_vcf_finish" in str(e.value) and ctx.last_vcf_handle is None, keys
    good = [Dl(0, 5, 2), Dl(0, 5, 3), Dl(0, 5, 94), In(0, 5, "A"), In(0, 5, "C"), In(0, 5, "A" * 25)]
    assert len(ctx.vcf_finish(ref, [k[0] for k in good], [k[1] for k in good], [1] * len(good), [0], [0], [9], 1, 0.0)["w0"]) == len(good)
    with pytest.raises(capi.MMError):
        ctx.vcf_finish(ref, [S(0, 5)[0]], [0], [1], [0], [5], [100], 1, 0.0)   # an interval past its contig's end
