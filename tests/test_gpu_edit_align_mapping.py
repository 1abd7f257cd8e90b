"""mm_mapping_align: the base-level alignment of every record of a mapping, the jobs made on the device from the records by the window and cap rules
(metamaps_amd/csrc/mm_edit.hip), on the small world of tests/test_gpu_edit_mapping.py: dist / first / last are mm_mapping_edit_distances', the runs are
those of the naive suffix table and its walk (tests/edit_cigar_ref.py) on the record's window.  Every comparison is exact."""
import numpy as np
import pytest

import edit_cigar_ref
import edit_ref
from test_gpu_edit_mapping import K, PI, W, world    # noqa: F401  (the fixture: this module gets a world of its own)

pytestmark = pytest.mark.gpu


def test_every_record_against_the_reference(world):
    ctx, rec = world["ctx"], world["rec"]
    idx = ctx.index(world["ref"], K, W)
    M = ctx.map_batch(idx, world["rd"], K, W, pi=PI)
    try:
        off, rec2 = M.fetch()
        assert np.array_equal(rec2, rec)
        dist, first, last, op_off, ops = ctx.mapping_align(M, world["rd"], world["ref"], PI)
    finally:
        M.close(); idx.close()
    assert list(zip(dist.tolist(), first.tolist(), last.tolist())) == world["got"]                     # what mapping_edit_distances gave
    assert len(op_off) == len(rec) + 1 and op_off[0] == 0 and op_off[-1] == len(ops)
    aligned = both = 0
    for k, r in enumerate(rec):
        read, contig = world["reads"][r["read"]], world["contigs"][r["ref_contig"]]
        ws, we = edit_ref.window(int(r["ref_start"]), len(read), len(contig))
        want = edit_cigar_ref.align(read, int(r["strand"]), contig[ws:we], edit_ref.cap(len(read), PI))
        runs = [int(w) for w in ops[op_off[k]:op_off[k + 1]]]
        if want is None:
            assert dist[k] == -1 and runs == []
            continue
        assert (int(dist[k]), int(first[k]), int(last[k])) == (want[0], ws + want[1], ws + want[2] - 1), (k, r)
        assert runs == want[3], (k, r, edit_cigar_ref.cigar(runs)[:200], edit_cigar_ref.cigar(want[3])[:200])
        edit_cigar_ref.check_invariants(read, int(r["strand"]), contig[ws:we], (want[0], want[1], want[2], runs))
        aligned += 1
        both += len(runs) > 50
    assert aligned >= 30 and both >= 10
