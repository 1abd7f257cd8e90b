"""mm_edit_infix_align (base-level alignments on the device: the storing pass of the bit-vector recurrence and the walk back, one job per wavefront;
metamaps_amd/csrc/mm_edit.hip, mm_edit_trace_core.hpp) through capi.py against the naive suffix table and its walk (tests/edit_cigar_ref.py): the edge
cases, the ladder of read lengths, the windows shorter than the pipeline, the built cases, 200 random problems in one call with their windows at
every phase of the 16-base packing, 0 jobs, one job three times, a scratch budget of 1 MB in a fresh process, the refusals and a read beyond the
longest.  Every comparison is exact."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import edit_bv_cases
import edit_cases
import edit_cigar_ref
import edit_ref
import edit_trace_cases
from test_gpu_edit_infix import BIG, Packed

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def answers(out):
    dist, begin, end, op_off, ops = out
    assert len(op_off) == len(dist) + 1 and op_off[0] == 0 and op_off[-1] == len(ops) and (np.diff(op_off) >= 0).all()
    return [None if d < 0 else (int(d), int(a), int(b), [int(w) for w in ops[o0:o1]]) for d, a, b, o0, o1 in zip(dist, begin, end, op_off[:-1], op_off[1:])]


def run_and_check(ctx, problems, want=None):
    pk = Packed(ctx, problems)
    try:
        out = ctx.edit_infix_align(pk.reads, pk.ref, **pk.jobs())
        plain = ctx.edit_infix(pk.reads, pk.ref, **pk.jobs())
    finally:
        pk.close()
    assert all(np.array_equal(x, y) for x, y in zip(out[:3], plain))          # dist / first / last are edit_infix's
    got = answers(out)
    want = [edit_cigar_ref.align(*p) for p in problems] if want is None else want
    for k, (g, x) in enumerate(zip(got, want)):
        where = (k, problems[k][1], len(problems[k][0]), len(problems[k][2]), problems[k][3])
        assert (g is None) == (x is None) and (g is None or g[:3] == x[:3]), where + (g and g[:3], x and x[:3])
        if g is not None:
            assert g[3] == x[3], where + (edit_cigar_ref.cigar(g[3])[:300], edit_cigar_ref.cigar(x[3])[:300])
            edit_cigar_ref.check_invariants(*problems[k][:3], g)
    dist, op_off = out[0], out[3]
    assert all(op_off[k] == op_off[k + 1] for k in range(len(dist)) if dist[k] < 0)   # not aligned: no runs
    return got


def random_problems():
    rng = np.random.default_rng(52)
    return [edit_cases.random_problem(rng, k) for k in range(200)]


def test_one_read_of_one_base(ctx):
    """the smallest job there is (the first one to run on a new machine)"""
    assert run_and_check(ctx, [(b"A", 1, b"A", None)]) == [(0, 0, 1, [1 << 4 | 7])]


def test_edges(ctx):
    problems = edit_cases.edge_problems(np.random.default_rng(7))
    got = run_and_check(ctx, problems)
    assert got[32:35] == [(20, 0, 0, [20 << 4 | 1]), None, (0, 0, 0, [])]
    assert [edit_cigar_ref.cigar(g[3]) for g in got[-3:]] == ["4=4X8=", "4I", "4=2X4="]
    got = run_and_check(ctx, list(edit_cases.at_cap_pair(np.random.default_rng(8))))
    assert got[1] is None and edit_cigar_ref.cigar(got[0][3]) == "5=1X11=1X11=1X11=1X11=1X6="


def test_block_ladder_short_windows_and_built_cases(ctx):
    built = edit_trace_cases.built_problems(np.random.default_rng(63))
    problems = edit_bv_cases.ladder_problems(np.random.default_rng(61)) + edit_bv_cases.short_window_problems(np.random.default_rng(62)) + built
    assert max(len(p[0]) for p in problems) == 128 * edit_bv_cases.W + 1
    got = run_and_check(ctx, problems)
    edit_trace_cases.check_built(built, got[-len(built):])
    assert sum(g is not None and len(g[3]) > 100 for g in got) >= 6


def test_200_random_problems_in_one_call(ctx):
    problems = random_problems()
    want = [edit_cigar_ref.align(*p) for p in problems]
    got = run_and_check(ctx, problems, want)
    assert sum(g is None for g in got) > 8 and sum(g is not None and g[0] > 0 for g in got) > 80
    pk = Packed(ctx, problems)
    try:
        order = [3, 17, 3, 3]                                                                             # one job three times in one call
        assert answers(ctx.edit_infix_align(pk.reads, pk.ref, **pk.jobs(order))) == [want[k] for k in order]
        none = ctx.edit_infix_align(pk.reads, pk.ref, **pk.jobs([]))                                      # no job: nothing is launched
        assert [len(x) for x in none] == [0, 0, 0, 1, 0] and none[3][0] == 0
    finally:
        pk.close()


CHILD = """
import pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import edit_bv_cases, test_gpu_edit_align as T
from test_gpu_edit_infix import Packed
from metamaps_amd import capi
ctx = capi.Context(0)
problems = T.random_problems() + edit_bv_cases.ladder_problems(np.random.default_rng(61))
pk = Packed(ctx, problems)
out = ctx.edit_infix_align(pk.reads, pk.ref, **pk.jobs())
pk.close(); ctx.close()
pickle.dump([x.tolist() for x in out], open(sys.argv[3], "wb"))
"""


def test_a_scratch_budget_of_1_mb_changes_nothing(ctx, tmp_path):
    """MM_EDIT_TRACE_MB=1: most jobs need far less, the reads of 2 047 bases and more need 1 to 7 MB each — many launches, and launches of one job
    that is larger than the budget.  The variable is read from the environment, hence the fresh process."""
    problems = random_problems() + edit_bv_cases.ladder_problems(np.random.default_rng(61))
    pk = Packed(ctx, problems)
    try:
        default = [x.tolist() for x in ctx.edit_infix_align(pk.reads, pk.ref, **pk.jobs())]
    finally:
        pk.close()
    assert "MM_EDIT_TRACE_MB" not in os.environ
    out = str(tmp_path / "small.pkl")
    p = subprocess.run([sys.executable, "-c", CHILD, HERE, os.path.dirname(HERE), out], env=dict(os.environ, MM_EDIT_TRACE_MB="1", MM_EDIT_TIMING="1"),
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    line = [x for x in p.stderr.decode().splitlines() if x.startswith("MM_EDIT_TIMING")][-1]
    assert "budget 1 MiB" in line and int(line.split(" launches")[0].split()[-1]) >= 12, line
    assert pickle.load(open(out, "rb")) == default


def test_refusals_leave_out_null(ctx):
    from metamaps_amd import capi
    pk = Packed(ctx, [(b"ACGTACGTAC", 1, b"ACGTACGTACGT", None), (b"ACGT", -1, b"ACGTT", None)])
    ok = dict(read=[0, 1], strand=[1, -1], contig=[0, 1], ws=[0, 1], we=[12, 6], max_dist=[5, 5])
    messages = {"read": "a read lies outside the read set", "contig": "a contig lies outside the reference set", "strand": "a strand is neither +1 nor -1",
                "max_dist": "a negative max_dist", "ws": "a window ends before it starts or lies outside its contig"}
    bad = [("read", 2), ("read", -1), ("contig", 2), ("contig", -1), ("strand", 0), ("strand", 2), ("max_dist", -1), ("ws", -1), ("ws", 7), ("we", pk.contig_len[1] + 1)]
    try:
        assert answers(ctx.edit_infix_align(pk.reads, pk.ref, **ok)) == [(0, 0, 10, [10 << 4 | 7]), (0, 0, 4, [4 << 4 | 7])]
        assert ctx.last_alignment_handle not in (None, 0xDEAD)
        for key, v in bad:
            args = {k: list(x) for k, x in ok.items()}
            args[key][1] = v                                        # the second job is the broken one: the first must not run either
            with pytest.raises(capi.MMError) as e:
                ctx.edit_infix_align(pk.reads, pk.ref, **args)
            assert e.value.status == -1 and messages["ws" if key == "we" else key] in str(e.value) and "mm_edit_infix_align" in str(e.value), (key, v, str(e.value))
            assert ctx.last_alignment_handle is None, (key, v)       # *out was set to NULL
    finally:
        pk.close()


def test_a_read_beyond_the_longest_has_no_runs(ctx):
    rng = np.random.default_rng(9)
    long_read = edit_cases.dna(rng, edit_ref.MAX_READ + 1)
    reads, ref = ctx.seqset([long_read, b"ACGTAC"]), ctx.seqset([long_read[:300]])
    try:
        got = answers(ctx.edit_infix_align(reads, ref, read=[0, 1, 0], strand=[1, 1, -1], contig=[0, 0, 0], ws=[0, 0, 0], we=[300, 300, 300], max_dist=[BIG, BIG, BIG]))
    finally:
        reads.close(); ref.close()
    want = edit_cigar_ref.align(b"ACGTAC", 1, long_read[:300])
    assert got == [None, want, None] and want is not None and len(want[3]) >= 1
