"""mm_edit_infix (exact edit distances on the device: Myers' bit-vector recurrence, one job per wavefront; metamaps_amd/csrc/mm_edit.hip) through capi.py
against the naive dynamic programme (tests/edit_ref.py): the edge cases, the ladder of read lengths at which a lane gets another block, 200 random problems in
one call with their windows at every phase of the 16-base packing, 0 and 1 jobs, one job twice, the refusals and a read beyond the longest.  Every
comparison is exact."""
import numpy as np
import pytest

import edit_bv_cases
import edit_cases
import edit_ref

pytestmark = pytest.mark.gpu
BIG = (1 << 31) - 1


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


class Packed:
    """the problems' reads as one set and their windows as another: window k lies at offset k % 18 inside its own contig, random bases around it"""

    def __init__(self, ctx, problems, seed=5):
        rng = np.random.default_rng(seed)
        self.problems = problems
        self.off = [k % 18 for k in range(len(problems))]
        contigs = [edit_cases.dna(rng, o) + p[2] + edit_cases.dna(rng, (7 * k) % 23) for k, (o, p) in enumerate(zip(self.off, problems))]
        self.reads, self.ref = ctx.seqset([p[0] for p in problems]), ctx.seqset(contigs)
        self.contig_len = [len(c) for c in contigs]

    def jobs(self, which=None):
        which = range(len(self.problems)) if which is None else which
        P = self.problems
        return dict(read=list(which), strand=[P[k][1] for k in which], contig=list(which), ws=[self.off[k] for k in which],
                    we=[self.off[k] + len(P[k][2]) for k in which], max_dist=[BIG if P[k][3] is None else P[k][3] for k in which])

    def close(self):
        self.reads.close(); self.ref.close()


def triples(out):
    dist, begin, end = out
    return [None if d < 0 else (int(d), int(a), int(b)) for d, a, b in zip(dist, begin, end)]


def run_and_check(ctx, problems, want=None):
    pk = Packed(ctx, problems)
    try:
        out = ctx.edit_infix(pk.reads, pk.ref, **pk.jobs())
    finally:
        pk.close()
    got = triples(out)
    want = [edit_ref.infix(*p) for p in problems] if want is None else want
    for k, (g, x) in enumerate(zip(got, want)):
        assert g == x, (k, problems[k][1], len(problems[k][0]), len(problems[k][2]), problems[k][3], g, x)
    assert all(a == -1 and b == -1 for d, a, b in zip(*out) if d < 0)
    return got


def test_one_read_of_one_base(ctx):
    """the smallest job there is (the first one to run on a new machine)"""
    assert run_and_check(ctx, [(b"A", 1, b"A", None)]) == [(0, 0, 1)]


def test_edges(ctx):
    problems = edit_cases.edge_problems(np.random.default_rng(7))
    got = run_and_check(ctx, problems)
    assert got[32:35] == [(20, 0, 0), None, (0, 0, 0)] and got[-3:] == [(4, 2, 18), (4, 0, 0), (2, 2, 12)]
    assert run_and_check(ctx, list(edit_cases.at_cap_pair(np.random.default_rng(8)))) == [(5, 20, 80), None]


def test_block_ladder_and_short_windows(ctx):
    problems = edit_bv_cases.ladder_problems(np.random.default_rng(61)) + edit_bv_cases.short_window_problems(np.random.default_rng(62))
    assert max(len(p[0]) for p in problems) == 128 * edit_bv_cases.W + 1
    got = run_and_check(ctx, problems)
    assert sum(g is not None and g[0] > 100 for g in got) >= 6


def test_200_random_problems_in_one_call_twice_each(ctx):
    rng = np.random.default_rng(52)
    problems = [edit_cases.random_problem(rng, k) for k in range(200)]
    want = [edit_ref.infix(*p) for p in problems]
    got = run_and_check(ctx, problems, want)
    assert sum(g is None for g in got) > 8 and sum(g is not None and g[0] > 0 for g in got) > 80
    pk = Packed(ctx, problems)
    try:
        assert triples(ctx.edit_infix(pk.reads, pk.ref, **pk.jobs([3]))) == [want[3]]                     # one job
        order = [int(k) for k in rng.permutation(200)] + [3, 3, 17]                                       # the same job several times in one call
        assert triples(ctx.edit_infix(pk.reads, pk.ref, **pk.jobs(order))) == [want[k] for k in order]
        none = ctx.edit_infix(pk.reads, pk.ref, **pk.jobs([]))                                            # no job: nothing is launched
        assert all(len(x) == 0 for x in none)
    finally:
        pk.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    from metamaps_amd import capi
    pk = Packed(ctx, [(b"ACGTACGTAC", 1, b"ACGTACGTACGT", None), (b"ACGT", -1, b"ACGTT", None)])
    ok = dict(read=[0, 1], strand=[1, -1], contig=[0, 1], ws=[0, 1], we=[12, 6], max_dist=[5, 5])
    messages = {"read": "a read lies outside the read set", "contig": "a contig lies outside the reference set", "strand": "a strand is neither +1 nor -1",
                "max_dist": "a negative max_dist", "ws": "a window ends before it starts or lies outside its contig"}
    bad = [("read", 2), ("read", -1), ("contig", 2), ("contig", -1), ("strand", 0), ("strand", 2), ("max_dist", -1), ("ws", -1), ("ws", 7), ("we", pk.contig_len[1] + 1)]
    try:
        assert triples(ctx.edit_infix(pk.reads, pk.ref, **ok)) == [edit_ref.infix(*p) for p in pk.problems] == [(0, 0, 10), (0, 0, 4)]
        for key, v in bad:
            args = {k: list(x) for k, x in ok.items()}
            args[key][1] = v                                        # the second job is the broken one: the first must not run either
            out = (np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int64), np.full(2, -7, dtype=np.int64))
            with pytest.raises(capi.MMError) as e:
                ctx.edit_infix(pk.reads, pk.ref, out=out, **args)
            assert e.value.status == -1 and messages["ws" if key == "we" else key] in str(e.value), (key, v, str(e.value))
            assert all((x == -7).all() for x in out)
    finally:
        pk.close()


def test_a_read_beyond_the_longest_is_not_aligned(ctx):
    rng = np.random.default_rng(9)
    long_read = edit_cases.dna(rng, edit_ref.MAX_READ + 1)
    reads, ref = ctx.seqset([long_read, b"ACGTAC"]), ctx.seqset([long_read[:300]])
    try:
        got = triples(ctx.edit_infix(reads, ref, read=[0, 1], strand=[1, 1], contig=[0, 0], ws=[0, 0], we=[300, 300], max_dist=[BIG, BIG]))
    finally:
        reads.close(); ref.close()
    assert got == [None, edit_ref.infix(b"ACGTAC", 1, long_read[:300])]
