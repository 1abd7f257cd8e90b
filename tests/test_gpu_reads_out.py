"""mm_reads_encode on the GPU, through capi.py, against tests/reads_out_ref.py: the inflated members of the edge set of tests/reads_out_cases.py — once as
an ASCII set and once as the same reads in BAM's 4-bit codes, added with reverse 0 and 1 (one set holds one kind) — for no, all, every third and a permuted
selection with repeats, as FASTA and FASTQ, under three group sizes; a set without a quality plane; every rule; a result of mm_seqset_hpc."""
import pytest

import bam_writer as bw
import reads_out_cases as cases
import reads_out_ref as ref

pytestmark = pytest.mark.gpu
MM_ERR_ARG, MM_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    assert hasattr(capi.lib(), "mm_reads_encode")
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    reads, quals = cases.edge_reads()
    S = ctx.seqset(reads, quals=[None if q is None else bytes(v + 33 for v in q) for q in quals], qual_offset=33)
    yield dict(reads=reads, quals=quals, set=S, names=cases.names_for(len(reads)))
    S.close()


@pytest.fixture(scope="module")
def world_nt16(ctx):
    """the reads of the edge set that BAM's alphabet holds, as 4-bit codes; every other record is stored as its reverse complement with its qualities
    reversed, and turned back by the set"""
    reads, quals = cases.edge_reads()
    keep = [i for i, r in enumerate(reads) if all(ch in bw.NT16 for ch in r.decode().upper())]
    reads = [reads[i].upper() for i in keep]; quals = [quals[i] for i in keep]
    assert len(reads) > 40 and any(b"N" in r for r in reads) and any(b"R" in r for r in reads)
    recs, rq = [], []
    for i, (r, q) in enumerate(zip(reads, quals)):
        rev = i % 2 == 1
        stored = bw.revcomp(r.decode()) if rev else r.decode()
        recs.append((bw.pack(stored), len(stored), rev))
        rq.append(None if q is None else bytes(reversed(q)) if rev else bytes(q))
    S = ctx.seqset_nt16(recs, quals=rq, qual_offset=0)
    yield dict(reads=reads, quals=quals, set=S, names=cases.names_for(len(reads)))
    S.close()


def _check(ctx, w, sel, with_qual, group_bytes=0):
    names = [w["names"][r] for r in sel]
    data, n_rec, raw = ctx.reads_encode(w["set"], sel, names, with_qual, group_bytes)
    want = ref.text(w["reads"], w["quals"], sel, names, with_qual)
    got = ref.inflate(data)
    assert n_rec == len(sel) and raw == len(want)
    assert got == want
    return data


@pytest.mark.parametrize("with_qual", [0, 1])
@pytest.mark.parametrize("which", ["none", "all", "every_third", "permuted_with_repeats"])
def test_selections_of_the_edge_set(ctx, world, which, with_qual):
    sel = cases.selections(len(world["reads"]))[which]
    data = _check(ctx, world, sel, with_qual)
    assert (data == b"") == (not sel)


@pytest.mark.parametrize("with_qual", [0, 1])
def test_nt16_reads_added_forward_and_reversed(ctx, world_nt16, with_qual):
    n = len(world_nt16["reads"])
    _check(ctx, world_nt16, list(range(n)), with_qual)
    _check(ctx, world_nt16, cases.selections(n)["permuted_with_repeats"], with_qual)


@pytest.mark.parametrize("with_qual", [0, 1])
def test_the_inflated_stream_does_not_depend_on_group_bytes(ctx, world, with_qual):
    sel = cases.selections(len(world["reads"]))["permuted_with_repeats"] * 4
    names = [world["names"][r] for r in sel]
    want = ref.text(world["reads"], world["quals"], sel, names, with_qual)
    assert len(want) > 65_280                                       # a record straddles two members
    largest = max(len(ref.record(nm, world["reads"][r], world["quals"][r], with_qual)) for r, nm in zip(sel, names))
    members = []
    for gb in (0, 1, largest - 1):                                  # the default; a cut between every two records; smaller than the largest record
        data = _check(ctx, world, sel, with_qual, gb)
        members.append(data)
    assert len(members[1]) > len(members[0])                        # (one member per record at least)


def test_with_qual_on_a_set_without_a_plane(ctx, world):
    S = ctx.seqset(world["reads"])
    try:
        w = dict(world, set=S, quals=[None] * len(world["reads"]))
        _check(ctx, w, list(range(len(world["reads"]))), 1)
        _check(ctx, w, list(range(len(world["reads"]))), 0)
    finally:
        S.close()


@pytest.mark.parametrize("rule,read,name", cases.bad_records())
def test_every_rule_names_the_lowest_bad_record(ctx, world, rule, read, name):
    from metamaps_amd import capi
    n = len(world["reads"])
    read = n if read == 3 else read                                  # (the cases speak of a set of 3 reads)
    good = world["names"][2]
    # a good record, the bad one, a good one, a record that breaks a lower-numbered rule, a good one
    later = (n + 7, b"x") if rule > 1 else (0, b"")                  # (behind rule 1 only a higher-numbered rule can follow)
    sel = [2, read, 4, later[0], 5]
    names = [good, name, b"ok", later[1], b"ok"]
    assert ref.refusal(sel, n, names) == (1, rule)
    with pytest.raises(capi.MMError) as e:
        ctx.reads_encode(world["set"], sel, names, 1)
    assert e.value.status == MM_ERR_ARG
    assert f"mm_reads_encode: record 1: rule {rule}:" in str(e.value)
    assert ctx.last_reads_text_handle is None
    _check(ctx, world, [2, 4, 5], 1)                                 # a following valid call works


def test_a_result_of_mm_seqset_hpc_is_refused(ctx, world):
    from metamaps_amd import capi
    H = world["set"].hpc()
    try:
        with pytest.raises(capi.MMError) as e:
            ctx.reads_encode(H, [0], [b"r"], 0)
        assert e.value.status == MM_ERR_STATE and "mm_seqset_hpc" in str(e.value)
        assert ctx.last_reads_text_handle is None
    finally:
        H.close()
    _check(ctx, world, [0, 1], 0)
