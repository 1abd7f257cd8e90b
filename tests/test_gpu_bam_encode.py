"""mm_bam_encode (BAM records encoded and deflated on the device: metamaps_amd/csrc/mm_bam.hip, mm_bam_core.hpp) through capi.py against the plain
restatement of the specification (tests/bam_ref.py), byte for byte: alignments that mm_edit_infix_align made (the built problems of the trace tests
and 40 random ones, some made unalignable), the built cases of tests/bam_cases.py as caller arrays (the 70 000-run job included), group sizes, two
calls, the members' container, 0 jobs and every refusal."""
import gzip
import struct

import numpy as np
import pytest

import bam_cases
import bam_ref
import edit_cases
import edit_trace_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def arrays(jobs, **over):
    """the call's arrays for jobs whose read and contig are entry k of their sets"""
    op_off = np.zeros(len(jobs) + 1, dtype=np.int64)
    np.cumsum([len(j["runs"]) for j in jobs], out=op_off[1:])
    a = dict(read=list(range(len(jobs))), strand=[j["strand"] for j in jobs], contig=list(range(len(jobs))), dist=[j["d"] for j in jobs], first=[j["first"] for j in jobs],
             op_off=op_off, ops=np.array([w for j in jobs for w in j["runs"]], dtype=np.uint32), flag=[j["flag"] for j in jobs], mapq=[j["mapq"] for j in jobs],
             names=[j["name"] for j in jobs])
    a.update(over)
    return a


@pytest.fixture(scope="module")
def built(ctx):
    """the built cases, their sets on the device and the reference's records: made once, never changed"""
    jobs = bam_cases.built_jobs()
    reads, ref = ctx.seqset([j["read"] for j in jobs]), ctx.seqset([j["contig"] for j in jobs])
    want = [bam_cases.record_of(bam_ref, j, k) for k, j in enumerate(jobs)]
    yield jobs, reads, ref, want
    reads.close(); ref.close()


def check_members(data):
    """every member is a BGZF block of at most 65 536 bytes that holds at most 65 280; returns their number"""
    ms = bam_ref.members(data)
    assert all(len(m) <= 65536 and len(raw) <= 65280 and struct.unpack_from("<I", m, len(m) - 4)[0] == len(raw) for m, raw in ms)
    return len(ms)


def test_alignments_from_the_device(ctx):
    rng = np.random.default_rng(81)
    problems = edit_trace_cases.built_problems(np.random.default_rng(63)) + [edit_cases.random_problem(rng, k) for k in range(40)]
    pad = [(k % 18, (7 * k) % 23) for k in range(len(problems))]
    contigs = [edit_cases.dna(rng, a) + p[2] + edit_cases.dna(rng, b) for (a, b), p in zip(pad, problems)]
    n = len(problems)
    max_dist = [(1 << 30) if p[3] is None else p[3] for p in problems]
    for k in (0, 1, 9, 14):                                         # reads with edits that may have none: not aligned, no record
        max_dist[k] = 0
    reads, ref = ctx.seqset([p[0] for p in problems]), ctx.seqset(contigs)
    try:
        dist, begin, end, op_off, ops = ctx.edit_infix_align(reads, ref, read=list(range(n)), strand=[p[1] for p in problems], contig=list(range(n)),
                                                             ws=[a for a, _ in pad], we=[a + len(p[2]) for (a, _), p in zip(pad, problems)], max_dist=max_dist)
        first = [a + int(b) if d >= 0 else -1 for (a, _), b, d in zip(pad, begin, dist)]
        flag = [(0x10 if p[1] < 0 else 0) | (0x100 if k % 2 else 0) for k, p in enumerate(problems)]
        mapq = [k % 61 for k in range(n)]
        names = [b"read_%d" % k for k in range(n)]
        data, n_rec, raw_bytes = ctx.bam_encode(reads, ref, read=list(range(n)), strand=[p[1] for p in problems], contig=list(range(n)), dist=dist, first=first,
                                                op_off=op_off, ops=ops, flag=flag, mapq=mapq, names=names)
    finally:
        reads.close(); ref.close()
    has = [d >= 0 and len(p[0]) > 0 for d, p in zip(dist, problems)]
    assert not has[0] and not has[1] and sum(has) >= 30 and sum(not h for h in has) >= 5
    want = b"".join(bam_ref.record(names[k], problems[k][0], problems[k][1], k, contigs[k], first[k], ops[op_off[k]:op_off[k + 1]], int(dist[k]), flag[k], mapq[k])
                    for k in range(n) if has[k])
    got = gzip.decompress(data) if data else b""
    assert got == want and n_rec == sum(has) and raw_bytes == len(want)
    assert {w & 15 for w in ops.tolist()} == {1, 2, 7, 8} and max(w >> 4 for w in ops.tolist() if w & 15 == 2) == 150
    check_members(data)


def test_built_cases_as_caller_arrays(ctx, built):
    jobs, reads, ref, want = built
    data, n_rec, raw_bytes = ctx.bam_encode(reads, ref, **arrays(jobs))
    got = gzip.decompress(data)
    at = 0
    for k, w in enumerate(want):                                    # record by record, so that a difference names its case
        assert got[at:at + len(w)] == w, (k, jobs[k]["name"])
        at += len(w)
    assert at == len(got) == raw_bytes and n_rec == len(jobs)
    assert {sum(len(w) for w in want[:k]) % 4 for k in range(len(want))} == {0, 1, 2, 3}


def test_group_sizes_and_two_calls(ctx, built):
    jobs, reads, ref, want = built
    small = [k for k, j in enumerate(jobs) if len(j["runs"]) < 100]  # (the long-CIGAR cases are ~1 MB each: one group each at any of these sizes)
    some = small + [k for k, j in enumerate(jobs) if j["name"] == b"runs65536"]
    a = arrays([jobs[k] for k in some], read=some, contig=some)
    whole = b"".join(want[k] for k in some)
    default, n_rec, raw = ctx.bam_encode(reads, ref, **a)
    again = ctx.bam_encode(reads, ref, **a)[0]
    assert again == default and gzip.decompress(default) == whole and (n_rec, raw) == (len(some), len(whole))
    n_default = check_members(default)
    for group_bytes in (4096, len(want[some[0]])):
        data = ctx.bam_encode(reads, ref, group_bytes=group_bytes, **a)[0]
        assert gzip.decompress(data) == whole
        assert check_members(data) > n_default, group_bytes


def test_no_jobs(ctx, built):
    jobs, reads, ref, want = built
    assert ctx.bam_encode(reads, ref, **arrays([])) == (b"", 0, 0)
    assert ctx.last_bam_handle not in (None, 0xDEAD)
    j = dict(jobs[0], d=-1, runs=[])
    assert ctx.bam_encode(reads, ref, **arrays([j])) == (b"", 0, 0)  # a job that is not aligned: no record, no member


def test_every_rule(ctx):
    from metamaps_amd import capi
    cases = bam_cases.broken_jobs()
    base = cases[0][0]
    good = bam_cases.job(b"first", base["contig"], 0, [(6, bam_cases.EQ)])
    reads, ref = ctx.seqset([good["read"], base["read"]]), ctx.seqset([good["contig"], base["contig"]])
    try:
        ok = ctx.bam_encode(reads, ref, **arrays([good, base]))
        assert gzip.decompress(ok[0]) == bam_cases.record_of(bam_ref, good, 0) + bam_cases.record_of(bam_ref, base, 1)
        for j, over, rule in cases:                                 # the second job is the broken one: the first must not come out either
            over = dict(over)
            idx = {k: [0, 2 if over.pop(k) > 0 else -1] for k in ("read", "contig") if k in over}   # (the sets here hold two sequences)
            with pytest.raises(capi.MMError) as e:
                ctx.bam_encode(reads, ref, **arrays([good, dict(base, **over)], **idx))
            assert e.value.status == -1 and "mm_bam_encode" in str(e.value) and f"job 1: rule {rule}:" in str(e.value), (over, rule, str(e.value))
            assert ctx.last_bam_handle is None, (over, rule)
    finally:
        reads.close(); ref.close()
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 3, 4, 5, 6, 7]
