"""The read-wise merge of per-chunk record lists (mm_merge.hip: mm_mapping_from_parts, mm_mapping_concat) against a numpy concatenation.
The parts are host arrays built here from fixed seeds: no index, no reads, no mapping run.  The kernels run 256-thread blocks, the count
kernel over n + 1 rows, so the read counts are 0, 1, 255, 256 and 257; the three-part cases hold one part without any record, every case
of 255 reads or more holds one read that is empty in every part, and every part has a contig base of its own."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, W, MIN_READ_LEN = 16, 8, 1000
READ_COUNTS = (0, 1, 255, 256, 257)
BASES = (5, 0, 1000)                                               # contig_base of part 0, 1, 2


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def read_lengths(n, seed):
    """lengths on both sides of min_read_len, and one below k and w"""
    return np.random.default_rng(seed).choice(np.array([7, 999, 1000, 1001, 5000], dtype=np.int32), size=n).astype(np.int32)


def make_part(n, seed, empty_read, no_records=False):
    """(offsets [n + 1], records) of one chunk: 0 .. 3 records per read, none for `empty_read`"""
    from metamaps_amd import capi
    rng = np.random.default_rng(seed)
    cnt = np.zeros(n, dtype=np.int64) if no_records else rng.integers(0, 4, size=n)
    if n > 1:
        cnt[empty_read] = 0
    elif n == 1 and not no_records:
        cnt[0] = 2
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    m = int(off[-1])
    rec = np.zeros(m, dtype=capi.RECORD_DTYPE)
    rec["read"] = np.repeat(np.arange(n), cnt)
    rec["ref_contig"] = rng.integers(0, 9, size=m); rec["ref_start"] = rng.integers(0, 1 << 30, size=m)
    rec["sketch"] = rng.integers(1, 500, size=m); rec["shared"] = rng.integers(0, 500, size=m)
    rec["strand"] = rng.choice([-1, 1], size=m); rec["mapq"] = rng.random(m)
    return off, rec


def numpy_merge(n, parts, bases):
    """read after read, part after part, ref_contig shifted by the part's base"""
    from metamaps_amd import capi
    shifted = []
    for (_, rec), b in zip(parts, bases):
        s = rec.copy(); s["ref_contig"] += b
        shifted.append(s)
    pieces = [s[int(off[r]):int(off[r + 1])] for r in range(n) for (off, _), s in zip(parts, shifted)]
    rec = np.concatenate(pieces) if pieces else np.zeros(0, dtype=capi.RECORD_DTYPE)
    off = np.zeros(n + 1, dtype=np.int64)
    for o, _ in parts:
        off += o
    return off, rec


def from_parts(ctx, read_len, parts, bases):
    """mm_mapping_from_parts through the library's own entry, the handle wrapped for fetch / stats / close"""
    from metamaps_amd import capi
    L = capi.lib()
    n = len(read_len)
    offs = [np.ascontiguousarray(o, dtype=np.int64) for o, _ in parts]
    recs = [np.ascontiguousarray(r, dtype=capi.RECORD_DTYPE) for _, r in parts]
    oarr = (C.c_void_p * len(parts))(*[o.ctypes.data for o in offs])
    rarr = (C.c_void_p * len(parts))(*[(r.ctypes.data if len(r) else None) for r in recs])
    base = np.asarray(bases, dtype=np.int32)
    mp = capi.MapParams(K, W, 80.0, MIN_READ_LEN)
    out = C.c_void_p()
    st = L.mm_mapping_from_parts(ctx.h, n, read_len.ctypes.data_as(C.c_void_p) if n else None, C.byref(mp), len(parts), oarr, rarr,
                                 base.ctypes.data_as(C.c_void_p), C.byref(out))
    assert st == 0, L.mm_last_error(ctx.h)
    assert out.value
    return capi.Mapping(ctx, out, n)


def check(M, read_len, want_off, want_rec):
    off, rec = M.fetch()
    assert np.array_equal(off, want_off)
    assert rec.tobytes() == want_rec.tobytes()                     # every field of every record, mapq bit for bit
    st = M.stats()
    assert st["n_reads"] == len(read_len)
    assert st["n_mappings"] == len(want_rec)
    assert st["n_reads_mapped"] == int(np.count_nonzero(np.diff(want_off)))
    assert st["n_reads_long_enough"] == int(np.count_nonzero(read_len >= max(K, W, MIN_READ_LEN)))


def case(n, n_parts, seed):
    parts = [make_part(n, seed + 10 * p, empty_read=n // 2, no_records=(n_parts == 3 and p == 1)) for p in range(n_parts)]
    return read_lengths(n, seed + 1), parts, BASES[:n_parts]


@pytest.mark.parametrize("n_parts", (1, 3))
@pytest.mark.parametrize("n", READ_COUNTS)
def test_from_parts_is_the_read_wise_concatenation(ctx, n, n_parts):
    read_len, parts, bases = case(n, n_parts, seed=1000 + n)
    want_off, want_rec = numpy_merge(n, parts, bases)
    if n >= 255:
        assert want_off[n // 2] == want_off[n // 2 + 1] and len(want_rec) > n      # (one read empty in every part; the case is no empty one)
    if n_parts == 3:
        assert parts[1][0][-1] == 0                                # (one part without any record)
    M = from_parts(ctx, read_len, parts, bases)
    try:
        check(M, read_len, want_off, want_rec)
    finally:
        M.close()


@pytest.mark.parametrize("n", READ_COUNTS)
def test_concat_of_two_merged_mappings(ctx, n):
    from metamaps_amd import capi
    L = capi.lib()
    read_len, parts_a, bases_a = case(n, 3, seed=2000 + n)
    _, parts_b, bases_b = case(n, 1, seed=3000 + n)
    A = from_parts(ctx, read_len, parts_a, bases_a)
    B = from_parts(ctx, read_len, parts_b, bases_b)
    try:
        halves = [numpy_merge(n, parts_a, bases_a), numpy_merge(n, parts_b, bases_b)]
        want_off, want_rec = numpy_merge(n, halves, (3, 40))
        arr = (C.c_void_p * 2)(A.h, B.h)
        base = np.array([3, 40], dtype=np.int32)
        out = C.c_void_p()
        st = L.mm_mapping_concat(ctx.h, arr, base.ctypes.data_as(C.c_void_p), 2, C.byref(out))
        assert st == 0, L.mm_last_error(ctx.h)
        M = capi.Mapping(ctx, out, n)
        try:
            check(M, read_len, want_off, want_rec)
        finally:
            M.close()
    finally:
        A.close(); B.close()
