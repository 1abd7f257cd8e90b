"""mm_consensus (the consensus of a group of contigs built on the device: metamaps_amd/csrc/mm_cons.hip, mm_cons_core.hpp) through capi.py against the plain
restatement tests/cons_ref.py: the built cases of tests/cons_cases.py and the 200 random tables (joined by their thresholds), once with one group per contig
and once with all contigs in one call, the threshold on the called positions, tables without rows or without intervals, and every refusal."""
import numpy as np
import pytest

import cons_cases
import cons_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def call(ctx, ref, w, lo, hi, **over):
    """mm_consensus on the rows and intervals of the contigs [lo, hi) of a world"""
    keys = [k for k in sorted(w["t"]) if lo <= k[0] >> 35 < hi]
    iv = [x for x in w["iv"] if lo <= x[0] < hi]
    p = dict(min_depth=w["D"], min_frac=w["F"], min_called=w["C"], line_width=w["width"])
    p.update(over)
    return ctx.consensus(ref, lo, hi, [k[0] for k in keys], [k[1] for k in keys], [w["t"][k] for k in keys], [c for c, _, _ in iv], [a for _, a, _ in iv], [b for _, _, b in iv], **p)


def as_dict(got):
    assert got["contig"].tolist() == sorted(set(got["contig"].tolist())) and set(got["written"].tolist()) == set(got["text"]) <= set(got["contig"].tolist())
    return {int(c): (s.tolist(), got["text"].get(int(c), b"")) for c, s in zip(got["contig"], got["stats"])}


def expected(w):
    res = cons_ref.consensus(w["t"], w["iv"], w["contigs"], w["D"], w["F"], w["C"])
    return {c: ([s[k] for k in cons_ref.STATS], cons_ref.wrapped(text, w["width"]).encode() if text is not None else b"") for c, (s, text, _) in res.items()}


def check_both_ways(ctx, w):
    """all contigs in one call, and one group per contig; returns what is expected"""
    want = expected(w)
    ref = ctx.seqset(w["contigs"])
    try:
        n = len(w["contigs"])
        assert as_dict(call(ctx, ref, w, 0, n)) == want
        each = {}
        for c in range(n):
            got = as_dict(call(ctx, ref, w, c, c + 1))
            assert set(got) <= {c}
            each.update(got)
        assert each == want
    finally:
        ref.close()
    return want


def test_built_cases(ctx):
    w = cons_cases.built_world()
    want = check_both_ways(ctx, w)
    c = {name: k for k, name in enumerate(cons_cases.CASES)}
    stat = lambda name, key: want[c[name]][0][cons_ref.STATS.index(key)]
    assert stat("d123", "deletions") == 3 and stat("d123", "dropped") == 2 and stat("big", "deletedBases") == 65535 + 64 + 65 and stat("big", "insertedBases") == 64 + 65 + 200
    assert c["no_intervals"] not in want and stat("nothing_called", "written") == 0 and want[c["nothing_called"]][1] == b""
    ref = ctx.seqset(w["contigs"])
    try:
        for width in (1, 7):                                        # other line widths, and a range in the middle
            assert as_dict(call(ctx, ref, w, 0, len(w["contigs"]), line_width=width)) == expected(dict(w, width=width)), width
        got = as_dict(call(ctx, ref, w, 3, 9))
        assert got == {k: v for k, v in want.items() if 3 <= k < 9} and len(got) == 6
    finally:
        ref.close()


def test_called_threshold(ctx):
    w = cons_cases.called_world()
    want = check_both_ways(ctx, w)
    assert [want[c][0][1:4] for c in (0, 1, 2)] == [[50, 1, 100], [50, 0, 0], [49, 0, 0]]


@pytest.mark.parametrize("combo", range(len(cons_cases.COMBOS)))
def test_random_tables(ctx, combo):
    worlds = cons_cases.random_worlds()
    assert len(worlds) == 200
    w = cons_cases.joined(worlds[combo::len(cons_cases.COMBOS)])
    want = check_both_ways(ctx, w)
    total = [sum(s[k] for s, _ in want.values()) for k in range(len(cons_ref.STATS))]
    assert min(total[cons_ref.STATS.index(k)] for k in ("snvs", "deletions", "insertions", "dropped", "written")) > 10, total


def test_nothing_and_intervals_only_and_rows_only(ctx):
    w = cons_cases.built_world()
    ref = ctx.seqset(w["contigs"])
    try:
        n = len(w["contigs"])
        got = call(ctx, ref, dict(w, t={}, iv=[]), 0, n)
        assert len(got["contig"]) == 0 and got["text"] == {} and ctx.last_cons_handle not in (None, 0xDEAD)
        assert len(call(ctx, ref, dict(w, iv=[]), 0, n)["contig"]) == 0                      # rows without any interval: no contig is reported
        assert len(call(ctx, ref, w, 5, 5)["contig"]) == 0                                   # an empty range
        only = dict(w, t={})
        assert as_dict(call(ctx, ref, only, 0, n)) == expected(only)
    finally:
        ref.close()


def test_refusals(ctx):
    from metamaps_amd import capi
    good, bad = cons_cases.refused_worlds()
    ref = ctx.seqset(good["contigs"])
    try:
        want = expected(good)
        assert as_dict(call(ctx, ref, good, 0, 2)) == want

        def refused(fn):
            with pytest.raises(capi.MMError) as e:
                fn()
            assert e.value.status == -1 and "mm_consensus" in str(e.value) and ctx.last_cons_handle is None, str(e.value)
            assert as_dict(call(ctx, ref, good, 0, 2)) == want      # a correct call follows on the same context
        for why, w in bad:
            keys = w.get("order") or sorted(w["t"])
            iv = w["iv"]
            refused(lambda: ctx.consensus(ref, 0, 2, [k[0] for k in keys], [k[1] for k in keys], [w["t"].get(k, 3) for k in keys], [c for c, _, _ in iv], [a for _, a, _ in iv],
                                          [b for _, _, b in iv], w["D"], w["F"], w["C"], w["width"]))
        refused(lambda: call(ctx, ref, dict(good, t={cons_cases.S(1, 3, "A"): 3}), 0, 2, line_width=0))
        # a row and an interval outside the range; a range outside the reference
        k = cons_cases.S(1, 3, "A")
        refused(lambda: ctx.consensus(ref, 0, 1, [k[0]], [k[1]], [3], [0], [0], [9]))
        refused(lambda: ctx.consensus(ref, 1, 2, [k[0]], [k[1]], [3], [0], [0], [9]))
        refused(lambda: ctx.consensus(ref, 0, 3, [k[0]], [k[1]], [3], [0], [0], [9]))
        refused(lambda: ctx.consensus(ref, 1, 0, [], [], [], [], [], []))
        refused(lambda: ctx.consensus(ref, -1, 1, [], [], [], [], [], []))
    finally:
        ref.close()
