"""The quality plane of a sequence set (mm_seqset_add_qual, mm_seqset_has_qual, mm_seqset_fetch_qual; the kernel of metamaps_amd/csrc/mm_seq.hip) through
capi.py: sequences around the 16-byte pieces a lane moves, ASCII with offset 33 and BAM's 4-bit codes with offset 0, forward and reversed, every second
sequence without qualities; slices and concatenations; every refusal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4097)
NT16 = "=ACMGRSVTWYHKDBN"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
ERR_ARG, ERR_DATA = -1, -8                                           # MM_ERR_ARG, MM_ERR_DATA


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def world(seed):
    """every length twice, so that each has a sequence with qualities and one without: (reads as ASCII, Phred bytes or None)"""
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for k, m in enumerate(LENGTHS + LENGTHS):
        reads.append(np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=m, p=[.24, .24, .24, .24, .04])].tobytes())
        quals.append(None if k % 2 else rng.integers(0, 94, size=m).astype(np.uint8).tobytes())
    return reads, quals


def nt16_record(read, reverse):
    """(4-bit codes, bases, reverse) as a BAM record holds the read: reverse-complemented where reverse is set"""
    s = read.decode()
    if reverse:
        s = "".join(COMP[ch] for ch in reversed(s))
    codes = [NT16.index(ch) for ch in s] + [0]
    return bytes(codes[2 * i] << 4 | codes[2 * i + 1] for i in range((len(s) + 1) // 2)), len(s), reverse


def check(S, reads, quals):
    assert S.count == len(reads)
    for i, (r, q) in enumerate(zip(reads, quals)):
        assert S.fetch(i, len(r)) == r, i
        assert S.fetch_qual(i, len(r)) == (b"\xff" * len(r) if q is None else q), (i, len(r))


def test_ascii_offset_33(ctx):
    from metamaps_amd import capi
    reads, quals = world(401)
    S = ctx.seqset(reads, quals=[None if q is None else bytes(b + 33 for b in q) for q in quals])
    plain = ctx.seqset(reads)
    try:
        assert S.has_qual and not plain.has_qual
        check(S, reads, quals)
        check(plain, reads, [None] * len(reads))                     # a set without a plane answers 0xFF
        assert S.fetch_range(0, S.count)[0].tobytes() == plain.fetch_range(0, S.count)[0].tobytes() == b"".join(reads)
    finally:
        S.close(); plain.close()


@pytest.mark.parametrize("reverse", [0, 1, "mixed"])
def test_nt16_offset_0(ctx, reverse):
    reads, quals = world(402)
    rev = [k % 3 == 0 if reverse == "mixed" else bool(reverse) for k in range(len(reads))]
    records = [nt16_record(r, v) for r, v in zip(reads, rev)]
    # a BAM record of a reversed read holds its qualities reversed as well
    S = ctx.seqset_nt16(records, quals=[None if q is None else (q[::-1] if v else q) for q, v in zip(quals, rev)])
    plain = ctx.seqset_nt16(records)
    try:
        assert S.has_qual and not plain.has_qual
        check(S, reads, quals)
        check(plain, reads, [None] * len(reads))
    finally:
        S.close(); plain.close()


def test_slice_and_concat_carry_the_plane(ctx):
    from metamaps_amd import capi
    reads, quals = world(403)
    S, plain = ctx.seqset(reads, quals=quals, qual_offset=0), ctx.seqset(reads[:5])
    made = []
    try:
        for first, count in ((0, len(reads)), (3, 7), (8, 1), (0, 0), (len(reads), 0)):
            T = S.slice(first, count); made.append(T)
            assert T.has_qual
            check(T, reads[first:first + count], quals[first:first + count])
        U = capi.SeqSet.concat(ctx, [made[1], plain, S, made[3]]); made.append(U)
        assert U.has_qual
        check(U, reads[3:10] + reads[:5] + reads, quals[3:10] + [None] * 5 + quals)
        V = capi.SeqSet.concat(ctx, [plain, plain]); made.append(V)
        W = plain.slice(1, 2); made.append(W)
        assert not V.has_qual and not W.has_qual
    finally:
        for T in made + [S, plain]:
            T.close()


@pytest.mark.parametrize("bad,offset", [(32, 33), (127, 33), (94, 0)])
def test_a_byte_out_of_range_is_a_data_error(ctx, bad, offset):
    """the lowest of two offending sequences is named, with its byte"""
    from metamaps_amd import capi
    reads, quals = world(404)
    raw = [None if q is None else bytearray(b + offset for b in q) for q in quals]
    for i, p in ((16, 32), (8, 4000), (6, 0)):                       # sequences of 33, 4097 and 32 bases; 6 is the lowest
        assert raw[i] is not None and len(raw[i]) > p
        raw[i][p] = bad
    with pytest.raises(capi.MMError) as e:
        ctx.seqset(reads, quals=raw, qual_offset=offset)
    assert e.value.status == ERR_DATA
    assert "sequence 6 " in str(e.value) and f"byte {bad}" in str(e.value)
    raw[6][0] = offset                                              # the next one up
    with pytest.raises(capi.MMError) as e:
        ctx.seqset(reads, quals=raw, qual_offset=offset)
    assert e.value.status == ERR_DATA and "sequence 8 " in str(e.value) and f"byte {bad}" in str(e.value)


def test_every_argument_refusal(ctx):
    from metamaps_amd import capi
    L = capi.lib()
    h = C.c_void_p()
    ctx.check(L.mm_seqset_create(ctx.h, C.byref(h)))
    S = capi.SeqSet(ctx, h)
    try:
        last = lambda: L.mm_last_error(ctx.h).decode()
        assert L.mm_seqset_has_qual(h) == 0
        assert L.mm_seqset_add_qual(h, b"II", 2, 33) == ERR_ARG and "no sequence" in last()      # no sequence yet
        ctx.check(L.mm_seqset_add(h, b"ACGT", 4))
        assert L.mm_seqset_add_qual(h, b"III", 3, 33) == ERR_ARG                                            # another length than the sequence's
        assert L.mm_seqset_add_qual(h, b"IIIII", 5, 33) == ERR_ARG
        for offset in (1, 32, 34, 64, -1):
            assert L.mm_seqset_add_qual(h, b"IIII", 4, offset) == ERR_ARG                                   # an offset that is not 0 or 33
        assert L.mm_seqset_has_qual(h) == 0
        ctx.check(L.mm_seqset_add_qual(h, b"IIII", 4, 33))
        assert L.mm_seqset_add_qual(h, b"IIII", 4, 33) == ERR_ARG and "already" in last()         # a second call for the same sequence
        ctx.check(L.mm_seqset_add(h, b"", 0))
        ctx.check(L.mm_seqset_add_qual(h, b"", 0, 33))
        assert L.mm_seqset_add_qual(h, b"", 0, 33) == ERR_ARG                                               # ... and for an empty one
        ctx.check(L.mm_seqset_add(h, b"GG", 2))
        assert L.mm_seqset_has_qual(h) == 1
        ctx.check(L.mm_seqset_upload(h))
        assert L.mm_seqset_add_qual(h, b"II", 2, 33) == ERR_ARG and "uploaded" in last()          # a frozen set
        assert S.has_qual and S.fetch_qual(0, 4) == bytes([40] * 4) and S.fetch_qual(2, 2) == b"\xff\xff"
        buf = np.zeros(8, dtype=np.uint8)
        assert L.mm_seqset_fetch_qual(h, 0, buf.ctypes.data_as(C.c_void_p), 3) == ERR_ARG                   # a buffer too small, an index out of range
        assert L.mm_seqset_fetch_qual(h, 3, buf.ctypes.data_as(C.c_void_p), 8) == ERR_ARG
        assert L.mm_seqset_fetch_qual(h, -1, buf.ctypes.data_as(C.c_void_p), 8) == ERR_ARG
    finally:
        S.close()
