"""mm_bam_encode_sorted and mm_bam_fetch_records (metamaps_amd/csrc/mm_bam.hip) through capi.py against tests/bam_ref.py: the built cases of
tests/bam_cases.py and 60 random ones laid onto three contigs in a shuffled order, jobs that share (contig, first), jobs that are not aligned.  The
inflated stream is the reference's records in ascending (contig, first, job), every record byte for byte the one mm_bam_encode writes; the records'
jobs and offsets are exact for both encoders; group sizes, 0 jobs and every refusal.  Then mm_bam_sorter_* (mm_bam_sort.hip) through capi.BamSorter on the
record sets of tests/bam_sort_cases.py: the merged file against the defined order, its members' sizes, three window sizes byte-identical, the .bai against
tests/bai_ref.py byte for byte, regions answered through the index against brute force, and every refusal."""
import gzip

import numpy as np
import pytest

import bai_ref
import bam_cases
import bam_ref
import bam_sort_cases
import bam_writer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def laid_out(jobs, n_contigs=3, seed=5):
    """the jobs on n_contigs contigs: every distinct contig of the jobs becomes a stretch of one of them, the stretches in a shuffled order, so that
    jobs with the same contig bytes and first share (contig, first).  Returns (contigs, jobs with contig index `c`, shifted first and the whole contig)."""
    rng = np.random.default_rng(seed)
    stretches = list(dict.fromkeys(j["contig"] for j in jobs))
    where, parts = {}, [[] for _ in range(n_contigs)]
    for s in rng.permutation(len(stretches)):
        c = int(s) % n_contigs
        where[stretches[s]] = (c, sum(len(p) for p in parts[c]))
        parts[c].append(stretches[s])
    contigs = [b"".join(p) for p in parts]
    out = []
    for j in jobs:
        c, base = where[j["contig"]]
        out.append(dict(j, c=c, first=base + j["first"], contig=contigs[c]))
    return contigs, out


def arrays(jobs, **over):
    op_off = np.zeros(len(jobs) + 1, dtype=np.int64)
    np.cumsum([len(j["runs"]) for j in jobs], out=op_off[1:])
    a = dict(read=list(range(len(jobs))), strand=[j["strand"] for j in jobs], contig=[j["c"] for j in jobs], dist=[j["d"] for j in jobs], first=[j["first"] for j in jobs],
             op_off=op_off, ops=np.array([w for j in jobs for w in j["runs"]], dtype=np.uint32), flag=[j["flag"] for j in jobs], mapq=[j["mapq"] for j in jobs],
             names=[j["name"] for j in jobs])
    a.update(over)
    return a


@pytest.fixture(scope="module")
def world(ctx):
    """the jobs, their sets on the device, the reference's record of every job (None: not aligned) and the defined order: made once, never changed"""
    contigs, jobs = laid_out(bam_cases.built_jobs() + bam_cases.random_jobs(60))
    for k in range(3, len(jobs), 7):                                # not aligned: no record
        jobs[k] = dict(jobs[k], d=-1, runs=[], first=-1)
    reads, ref = ctx.seqset([j["read"] for j in jobs]), ctx.seqset(contigs)
    want = [None if j["d"] < 0 else bam_ref.record(j["name"], j["read"], j["strand"], j["c"], j["contig"], j["first"], j["runs"], j["d"], j["flag"], j["mapq"]) for j in jobs]
    order = sorted((k for k in range(len(jobs)) if want[k] is not None), key=lambda k: (jobs[k]["c"], jobs[k]["first"], k))
    yield jobs, reads, ref, want, order
    reads.close(); ref.close()


def offsets(want, order):
    return np.concatenate([[0], np.cumsum([len(want[k]) for k in order])]).astype(np.int64)


def test_the_cases_are_the_ones_asked_for(world):
    jobs, _, _, want, order = world
    keys = [(jobs[k]["c"], jobs[k]["first"]) for k in order]
    assert {c for c, _ in keys} == {0, 1, 2} and len(keys) - len(set(keys)) >= 10           # three contigs; jobs that share (contig, first)
    assert sum(w is None for w in want) >= 10 and order != sorted(order)                       # jobs without a record; an order that is not the jobs'
    assert max(len(w) for w in want if w) > 3 * 65280                                          # a record longer than three members
    assert {int(o) % 4 for o in offsets(want, order)} == {0, 1, 2, 3}


def test_sorted_stream_and_records(ctx, world):
    jobs, reads, ref, want, order = world
    data, n_rec, raw_bytes = ctx.bam_encode_sorted(reads, ref, **arrays(jobs))
    got, at = gzip.decompress(data), 0
    for k in order:                                                 # record by record, so that a difference names its case
        assert got[at:at + len(want[k])] == want[k], (k, jobs[k]["name"])
        at += len(want[k])
    assert at == len(got) == raw_bytes and n_rec == len(order)
    again, job, raw_off = ctx.bam_records(reads, ref, sorted=True, **arrays(jobs))
    assert again == data and job.tolist() == order and np.array_equal(raw_off, offsets(want, order))
    ms = bam_ref.members(data)
    assert all(len(m) <= 65536 and len(raw) <= 65280 for m, raw in ms)


def test_unsorted_encoder_is_what_it_was_and_names_its_records(ctx, world):
    jobs, reads, ref, want, order = world
    in_jobs = sorted(order)
    data, job, raw_off = ctx.bam_records(reads, ref, **arrays(jobs))
    assert gzip.decompress(data) == b"".join(want[k] for k in in_jobs)
    assert job.tolist() == in_jobs and np.array_equal(raw_off, offsets(want, in_jobs))
    assert ctx.bam_encode(reads, ref, **arrays(jobs))[0] == data


def test_group_sizes(ctx, world):
    jobs, reads, ref, want, order = world
    small = [k for k in range(len(jobs)) if len(jobs[k]["runs"]) < 100]   # (the long-CIGAR records are ~1 MB each)
    a = arrays([jobs[k] for k in small], read=small)
    sub = [i for i in sorted(range(len(small)), key=lambda i: (jobs[small[i]]["c"], jobs[small[i]]["first"], i)) if want[small[i]] is not None]
    whole = b"".join(want[small[i]] for i in sub)
    default = ctx.bam_encode_sorted(reads, ref, **a)[0]
    assert gzip.decompress(default) == whole
    for group_bytes in (4096, 36):                                  # groups of a few records, and of one record each
        data, job, raw_off = ctx.bam_records(reads, ref, sorted=True, group_bytes=group_bytes, **a)
        assert gzip.decompress(data) == whole and job.tolist() == sub, group_bytes
        assert len(bam_ref.members(data)) > len(bam_ref.members(default))


def test_no_jobs_and_no_records(ctx, world):
    jobs, reads, ref, _, _ = world
    none = arrays([])
    assert ctx.bam_encode_sorted(reads, ref, **none) == (b"", 0, 0)
    assert ctx.last_bam_handle not in (None, 0xDEAD)
    for is_sorted in (False, True):
        data, job, raw_off = ctx.bam_records(reads, ref, sorted=is_sorted, **none)
        assert data == b"" and job.tolist() == [] and raw_off.tolist() == [0]
        data, job, raw_off = ctx.bam_records(reads, ref, sorted=is_sorted, **arrays([dict(jobs[0], d=-1, runs=[])]))
        assert data == b"" and job.tolist() == [] and raw_off.tolist() == [0]


def test_every_rule_of_the_unsorted_encoder(ctx):
    from metamaps_amd import capi
    cases = bam_cases.broken_jobs()
    base = dict(cases[0][0], c=1)
    good = dict(bam_cases.job(b"first", base["contig"], 0, [(6, bam_cases.EQ)]), c=0)
    reads, ref = ctx.seqset([good["read"], base["read"]]), ctx.seqset([good["contig"], base["contig"]])
    try:
        ok = ctx.bam_encode_sorted(reads, ref, **arrays([good, base]))
        assert gzip.decompress(ok[0]) == bam_cases.record_of(bam_ref, good, 0) + bam_cases.record_of(bam_ref, base, 1)
        for j, over, rule in cases:                                 # the second job is the broken one: the first must not come out either
            over = dict(over)
            idx = {k: [0, 2 if over.pop(k) > 0 else -1] for k in ("read", "contig") if k in over}   # (the sets here hold two sequences)
            with pytest.raises(capi.MMError) as e:
                ctx.bam_encode_sorted(reads, ref, **arrays([good, dict(base, **over)], **idx))
            assert e.value.status == -1 and "mm_bam_encode_sorted" in str(e.value) and f"job 1: rule {rule}:" in str(e.value), (over, rule, str(e.value))
            assert ctx.last_bam_handle is None, (over, rule)
        with pytest.raises(capi.MMError) as e:
            ctx.bam_encode_sorted(reads, ref, group_bytes=-1, **arrays([good, base]))
        assert e.value.status == -1 and "group_bytes" in str(e.value)
    finally:
        reads.close(); ref.close()
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 3, 4, 5, 6, 7]


# ---- the sorter: mm_bam_sorter_* (metamaps_amd/csrc/mm_bam_sort.hip) against tests/bai_ref.py, on the record sets of tests/bam_sort_cases.py ----
MEMBER = bam_sort_cases.MEMBER
CASES = {"edges": bam_sort_cases.edges, "ties": bam_sort_cases.ties, "one_run": bam_sort_cases.one_run, "nothing": bam_sort_cases.nothing}


def header_members(case):
    return bam_writer.bgzf_block(bam_sort_cases.header(case["ref_len"]))


def sort_file(ctx, case, window_bytes):
    """(the .bam's bytes, the .bai's bytes, number of windows) of a case through capi.BamSorter"""
    from metamaps_amd import capi
    s = capi.BamSorter(ctx, case["ref_len"], window_bytes)
    try:
        for run in case["runs"]:
            s.add_run(*bam_sort_cases.run_arrays(run))
        n_windows, stream_bytes = s.plan()
        assert stream_bytes == sum(len(rec) for run in case["runs"] for rec in run)
        head = header_members(case)
        body = b"".join(s.window(w) for w in range(n_windows))
        return head + body + bam_ref.EOF_BLOCK, s.index(len(head)), n_windows
    finally:
        s.close()


@pytest.fixture(scope="module")
def sorted_files(ctx):
    """(the cases, the files made of them so far by (case, window_bytes)): made() sorts a case the first time it is asked for and keeps the result"""
    return {name: (make(), ) for name, make in CASES.items()}, {}


def made(ctx, sorted_files, name, window_bytes=0):
    cases, files = sorted_files
    if (name, window_bytes) not in files:
        files[(name, window_bytes)] = sort_file(ctx, cases[name][0], window_bytes)
    return cases[name][0], files[(name, window_bytes)]


def test_the_record_sets_are_the_ones_asked_for():
    case = bam_sort_cases.edges()
    stream = bam_sort_cases.sorted_stream(case)
    ends = np.cumsum([len(r) for r in stream])
    assert {int(e) % MEMBER for e in ends} >= {0, 1, MEMBER - 1}                          # a record's end on a member's edge and to either side of it
    sizes = {len(r) for r in stream}
    assert min(sizes) == 36 and MEMBER + 1 in sizes and 3 * MEMBER + 1 in sizes
    src = [int(o) % 4 for run in case["runs"] for o in np.cumsum([0] + [len(r) for r in run])[:-1]]
    place = {id(r): int(o) % 4 for r, o in zip(stream, np.concatenate([[0], ends[:-1]]))}
    dst = [place[id(r)] for run in case["runs"] for r in run]
    assert len(set(zip(src, dst))) == 16                            # every source residue against every destination residue
    refs = {c[0] for r in stream for c in bam_sort_cases.coords(r)}
    assert refs == {0, 2, 4} and {(1 << 29) - 2, 1 << 26, 1 << 17, 1 << 14, (1 << 14) - 1, 0} <= {c[1] for r in stream for c in bam_sort_cases.coords(r)}
    t = bam_sort_cases.ties()
    assert len(t["runs"]) == 17 and any(not r for r in t["runs"]) and len({bam_sort_cases.coords(rec)[0][:2] for r in t["runs"] for rec in r}) == 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_sorted_file_and_index(ctx, sorted_files, name):
    case, (bam, bai, n_windows) = made(ctx, sorted_files, name)
    want = b"".join(bam_sort_cases.sorted_stream(case))
    head = header_members(case)
    ms = bam_ref.members(bam[len(head):])
    assert b"".join(raw for _, raw in ms) == want
    assert all(len(raw) == MEMBER for _, raw in ms[:-2]) and ms[-1][0] == bam_ref.EOF_BLOCK and (len(ms) == 1 or 0 < len(ms[-2][1]) <= MEMBER)
    assert gzip.decompress(bam) == gzip.decompress(head) + want
    assert n_windows == (1 if want else 0)
    assert bai == bai_ref.build(bam, bam_sort_cases.coords)
    if not want:
        assert all(x == dict(bins={}, pseudo=None, ioff=[]) for x in bai_ref.parse(bai)) and bam == head + bam_ref.EOF_BLOCK


@pytest.mark.parametrize("name", ["edges", "ties", "one_run"])
def test_the_window_does_not_show_in_the_files(ctx, sorted_files, name):
    case, (bam, bai, _) = made(ctx, sorted_files, name)
    for window_bytes in (MEMBER, 2 * MEMBER):
        bam_w, bai_w, n_windows = sort_file(ctx, case, window_bytes)
        assert n_windows == -(-sum(len(rec) for run in case["runs"] for rec in run) // window_bytes)
        assert bam_w == bam and bai_w == bai, window_bytes


@pytest.mark.parametrize("name", ["edges", "one_run"])
def test_regions_through_the_index(ctx, sorted_files, name):
    case, (bam, bai, _) = made(ctx, sorted_files, name)
    _, recs = bai_ref.placed(bam, bam_sort_cases.coords)
    idx = bai_ref.parse(bai)
    regions = bam_sort_cases.regions(case)
    assert len(regions) >= 300
    hits = 0
    for ref, beg, end in regions:
        chunks = bai_ref.query(idx, ref, beg, end)
        got = [k for k, (r, b, e, vs, ve) in enumerate(recs) if any(a <= vs < z for a, z in chunks) and r == ref and b < end and e > beg]
        brute = [k for k, (r, b, e, vs, ve) in enumerate(recs) if r == ref and b < end and e > beg]
        assert got == brute, (ref, beg, end)
        hits += len(brute)
    assert hits > 100


def test_sorter_refusals(ctx):
    from metamaps_amd import capi
    rng = np.random.default_rng(3)
    rec = lambda ref, pos, end, size=40: bam_sort_cases.record(rng, ref, pos, end, size)
    good = [rec(0, 1, 5), rec(0, 7, 9), rec(1, 0, 3)]
    bgzf, raw_off, ref, pos, end = bam_sort_cases.run_arrays(good)

    def refused(status, *words, **over):
        a = dict(bgzf=bgzf, raw_off=raw_off, ref_id=ref, pos=pos, end=end); a.update(over)
        s = capi.BamSorter(ctx, [10, 10])
        try:
            s.add_run(*bam_sort_cases.run_arrays(good[:1]))         # run 0 is fine: the refusal names run 1
            with pytest.raises(capi.MMError) as e:
                s.add_run(**a)
                n = s.plan()[0]
                [s.window(w) for w in range(n)]
            assert e.value.status == status and all(w in str(e.value) for w in words), str(e.value)
        finally:
            s.close()
    refused(-1, "run 1", "record 1", "not sorted", pos=[8, 7, 0], end=[9, 9, 3])
    refused(-1, "run 1", "record 2", "not sorted", ref_id=[0, 1, 0], pos=[1, 0, 0], end=[5, 3, 3])
    refused(-1, "run 1", "record 3", "raw_off", raw_off=[0, 40, 80, 121])
    refused(-1, "run 1", "record 1", "raw_off", raw_off=[0, 80, 80, 120])
    refused(-1, "run 1", "record 2", "ref_id", ref_id=[0, 0, 2])
    refused(-1, "run 1", "record 0", "ref_id", ref_id=[-1, 0, 1])
    refused(-1, "run 1", "record 0", "pos", pos=[-1, 7, 0])
    refused(-1, "run 1", "record 2", "end", end=[5, 9, 11])
    broken = bytearray(bgzf); broken[20] ^= 0x5A; broken[21] ^= 0xA5                      # inside the member's deflate stream
    refused(-8, "run 1", "member 0", "does not inflate", bgzf=bytes(broken))
    for ref_len, window in (([10, 1 << 29], 0), ([10], 1000), ([10], -MEMBER)):
        with pytest.raises(capi.MMError) as e:
            capi.BamSorter(ctx, ref_len, window)
        assert e.value.status == -1 and "mm_bam_sorter_create" in str(e.value)
    import ctypes as C
    long_contig, h = np.array([1 << 29], dtype=np.int32), C.c_void_p(0xDEAD)
    assert capi.lib().mm_bam_sorter_create(ctx.h, 1, long_contig.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == -1 and h.value is None   # (*out is NULL after a refusal)
    s = capi.BamSorter(ctx, [10, 10], MEMBER)
    try:
        s.add_run(bgzf, raw_off, ref, pos, end)
        with pytest.raises(capi.MMError) as e:
            s.window(0)                                             # before the plan
        assert e.value.status == -4
        assert s.plan() == (1, 120)
        with pytest.raises(capi.MMError) as e:
            s.index(0)                                              # before the last window
        assert e.value.status == -4
        assert len(s.window(0)) > 28 and len(s.index(0)) > 8
    finally:
        s.close()
