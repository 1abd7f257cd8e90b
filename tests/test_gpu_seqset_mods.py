"""The modification plane of a sequence set (mm_seqset_add_mods, mm_seqset_has_mods, mm_seqset_fetch_mods; mod_plane_kernel of
metamaps_amd/csrc/mm_mods.hip) through capi.py against tests/mods_ref.py on the plane cases of tests/mods_cases.py: ASCII and BAM's 4-bit codes, forward,
reversed and mixed, every second read without groups; slices and concatenations; the data error with its message; every argument refusal."""
import numpy as np
import pytest

import mods_cases
import mods_ref

pytestmark = pytest.mark.gpu

NT16 = "=ACMGRSVTWYHKDBN"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "R": "Y"}
ERR_ARG, ERR_DATA = -1, -8                                           # MM_ERR_ARG, MM_ERR_DATA


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def good():
    """the plane cases without an error, each followed by its read without groups: (reads, groups or None, planes)"""
    reads, groups, planes = [], [], []
    for name, read, g, bad in mods_cases.plane_cases():
        if bad is None:
            reads += [read, read]; groups += [g, None]
            planes += [mods_ref.plane(read, g), (bytes(len(read)), bytes(len(read)))]
    return reads, groups, planes


def nt16_record(read, reverse):
    """(4-bit codes, bases, reverse) as a BAM record holds the read: reverse-complemented where reverse is set"""
    s = read.decode().upper()
    if reverse:
        s = "".join(COMP[ch] for ch in reversed(s))
    codes = [NT16.index(ch) for ch in s] + [0]
    return bytes(codes[2 * i] << 4 | codes[2 * i + 1] for i in range((len(s) + 1) // 2)), len(s), reverse


def check(S, reads, planes, first=0):
    for i, (r, p) in enumerate(zip(reads, planes)):
        assert S.fetch_mods(first + i, len(r)) == p, (first + i, len(r))


def test_ascii(ctx, good):
    reads, groups, planes = good
    S, plain = ctx.seqset(reads, mods=groups), ctx.seqset(reads)
    try:
        assert S.has_mods and not plain.has_mods and S.count == len(reads)
        check(S, reads, planes)
        check(plain, reads, [(bytes(len(r)), bytes(len(r))) for r in reads])   # a set without a plane answers zeros
        assert all(S.fetch(i, len(r)) == r.upper() for i, r in enumerate(reads))
        assert any(set(w) >= {1, 3} for w, _ in planes) and any(2 in w for w, _ in planes) and any(4 in w for w, _ in planes)
    finally:
        S.close(); plain.close()


@pytest.mark.parametrize("which", ["forward", "reversed", "mixed"])
def test_nt16(ctx, good, which):
    reads, groups, planes = good
    rev = [dict(forward=0, reversed=1, mixed=(i // 2) % 2)[which] for i in range(len(reads))]
    S = ctx.seqset_nt16([nt16_record(r, v) for r, v in zip(reads, rev)], mods=groups)
    try:
        assert S.has_mods
        check(S, reads, planes)                                      # the groups speak of the read as sequenced, which is what the set holds
    finally:
        S.close()


def test_slice_and_concat_carry_the_planes(ctx, good):
    from metamaps_amd import capi
    reads, groups, planes = good
    S, plain = ctx.seqset(reads, mods=groups), ctx.seqset(reads[:5])
    parts = []
    try:
        n = len(reads)
        for first, count in ((0, n), (3, 7), (n - 1, 1), (4, 0)):
            parts.append(S.slice(first, count))
            assert parts[-1].has_mods
            check(parts[-1], reads[first:first + count], planes[first:first + count])
        cat = capi.SeqSet.concat(ctx, [parts[1], plain, parts[2]])
        parts.append(cat)
        assert cat.has_mods
        check(cat, reads[3:10] + reads[:5] + reads[n - 1:], planes[3:10] + [(bytes(len(r)), bytes(len(r))) for r in reads[:5]] + planes[n - 1:])
        none = capi.SeqSet.concat(ctx, [plain, plain])
        parts.append(none)
        assert not none.has_mods
    finally:
        for p in parts + [S, plain]:
            p.close()


def test_the_data_error_names_the_lowest_sequence_and_group(ctx):
    from metamaps_amd import capi
    cases = {name: (read, g) for name, read, g, bad in mods_cases.plane_cases()}
    ok = cases["edges_129"]
    reads = [ok[0], ok[0], cases["beyond_second_group_65"][0], ok[0], cases["beyond_4097"][0], cases["huge_skips"][0]]
    groups = [ok[1], None, cases["beyond_second_group_65"][1], ok[1], cases["beyond_4097"][1], cases["huge_skips"][1]]
    with pytest.raises(capi.MMError) as e:
        ctx.seqset(reads, mods=groups)
    assert e.value.status == ERR_DATA and "mm_seqset_upload: sequence 2: modification group 1 names more G bases" in str(e.value), str(e.value)
    with pytest.raises(capi.MMError) as e:
        ctx.seqset(reads[3:], mods=groups[3:])
    assert e.value.status == ERR_DATA and "sequence 1: modification group 0 names more C bases" in str(e.value), str(e.value)
    S = ctx.seqset(reads[:2] + reads[3:4], mods=groups[:2] + groups[3:4])   # the same set without the offenders
    try:
        assert S.fetch_mods(2, len(ok[0])) == mods_ref.plane(*ok)
    finally:
        S.close()


def test_every_argument_refusal(ctx):
    import ctypes as C
    from metamaps_amd import capi
    L = capi.lib()
    g = dict(base="C", code=0, mode="?", skips=[0], ml=[200])

    def fresh():
        h = C.c_void_p()
        ctx.check(L.mm_seqset_create(ctx.h, C.byref(h)))
        return h

    def refused(h, groups, what, **over):
        with pytest.raises(capi.MMError) as e:
            ctx.add_mods(h, groups, **over)
        assert e.value.status == ERR_ARG and "mm_seqset_add_mods: " in str(e.value) and what in str(e.value), (what, str(e.value))

    h = fresh()
    try:
        refused(h, [g], "no sequence yet")
        ctx.check(L.mm_seqset_add(h, b"ACCA", 4))
        refused(h, [dict(g, base="N")], "not one of A C G T")
        refused(h, [dict(g, base="c")], "not one of A C G T")
        refused(h, [dict(g, code=4)], "not in [-1, 3]")
        refused(h, [dict(g, code=-2)], "not in [-1, 3]")
        refused(h, [dict(g, mode="!")], "mode")
        refused(h, [g, g], "falls", off=np.array([0, 1, 0], dtype=np.int64))
        refused(h, [g], "falls", off=np.array([-1, 0], dtype=np.int64))
        refused(h, [g], "n_groups", n_groups=256)
        refused(h, [g], "n_groups", n_groups=-1)
        assert L.mm_seqset_add_mods(h, 1, None, None, None, None, None, None) == ERR_ARG
        assert L.mm_seqset_add_mods(None, 0, None, None, None, None, None, None) == ERR_ARG
        assert not L.mm_seqset_has_mods(h)                           # a refused call leaves nothing behind
        ctx.add_mods(h, [g, dict(g, code=-1, mode="")])
        assert L.mm_seqset_has_mods(h)
        refused(h, [g], "already")                                   # a second call for one sequence
        ctx.check(L.mm_seqset_add(h, b"GG", 2))
        ctx.add_mods(h, [])                                          # no groups: a row of zeros
        ctx.check(L.mm_seqset_upload(h))
        refused(h, [g], "already uploaded")
        S = capi.SeqSet(ctx, h)
        assert S.has_mods and S.fetch_mods(0, 4) == mods_ref.plane(b"ACCA", [g, dict(g, code=-1, mode="")]) and S.fetch_mods(1, 2) == (bytes(2), bytes(2))
        with pytest.raises(capi.MMError):
            S.fetch_mods(2, 4)
        with pytest.raises(capi.MMError):
            S.fetch_mods(0, 3)                                       # cap below the length
    finally:
        L.mm_seqset_destroy(h)
