"""QUAL in the records of mm_bam_encode (metamaps_amd/csrc/mm_bam.hip, mm_bam_core.hpp) through capi.py: the built jobs of tests/bam_cases.py with a read set
whose qualities are (7 i + r) mod 94 for base i of read r, every fifth read without.  Every record's QUAL is tests/qual_ref.py's, and with QUAL blanked the
inflated stream is that of the same call on a set without qualities."""
import gzip

import numpy as np
import pytest

import bam_cases
import bam_ref
import qual_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def arrays(jobs):
    op_off = np.zeros(len(jobs) + 1, dtype=np.int64)
    np.cumsum([len(j["runs"]) for j in jobs], out=op_off[1:])
    return dict(read=list(range(len(jobs))), strand=[j["strand"] for j in jobs], contig=list(range(len(jobs))), dist=[j["d"] for j in jobs], first=[j["first"] for j in jobs],
                op_off=op_off, ops=np.array([w for j in jobs for w in j["runs"]], dtype=np.uint32), flag=[j["flag"] for j in jobs], mapq=[j["mapq"] for j in jobs],
                names=[j["name"] for j in jobs])


def test_qual_of_every_built_record(ctx):
    jobs = bam_cases.built_jobs()
    quals = [None if r % 5 == 4 else bytes((7 * i + r) % 94 for i in range(len(j["read"]))) for r, j in enumerate(jobs)]
    reads_q, reads, ref = ctx.seqset([j["read"] for j in jobs], quals=quals, qual_offset=0), ctx.seqset([j["read"] for j in jobs]), ctx.seqset([j["contig"] for j in jobs])
    try:
        assert reads_q.has_qual and not reads.has_qual
        with_q, n_q, raw_q = ctx.bam_encode(reads_q, ref, **arrays(jobs))
        without, n, raw = ctx.bam_encode(reads, ref, **arrays(jobs))
    finally:
        reads_q.close(); reads.close(); ref.close()
    got, plain = gzip.decompress(with_q), gzip.decompress(without)
    assert (n_q, raw_q) == (n, raw) == (len(jobs), len(got)) and len(got) == len(plain)
    recs = bam_ref.decode_records(got)
    assert len(recs) == len(jobs)
    for r, (rec, j, q) in enumerate(zip(recs, jobs, quals)):
        assert rec["qual"] == qual_ref.bam_qual(dict(j, qual=q)), (r, j["name"])
        if q is None:
            assert rec["qual"] == b"\xff" * len(j["read"])
    assert {j["strand"] for j, q in zip(jobs, quals) if q is not None and len(q) > 1} == {1, -1}
    assert any(q is None for q in quals) and got != plain
    # QUAL blanked: every other byte is that of the call without qualities, which tests/test_gpu_bam_encode.py holds to bam_ref
    blank, at = bytearray(got), 0
    for j in jobs:
        w = bam_cases.record_of(bam_ref, j, 0)
        field = min(len(j["runs"]), 65535) if len(j["runs"]) <= 65535 else 2
        qat = at + 36 + len(j["name"]) + 1 + 4 * field + (len(j["read"]) + 1) // 2
        blank[qat:qat + len(j["read"])] = b"\xff" * len(j["read"])
        at += len(w)
    assert at == len(got) and bytes(blank) == plain
