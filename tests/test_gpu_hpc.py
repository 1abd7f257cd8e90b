"""Homopolymer compression on the device at the ABI level: mm_seqset_hpc against the definition (every maximal run of equal bytes, as hashed —
upper-cased, IUPAC and N kept — becomes one byte), its coordinate map against the definition of raw / rawlast, and the compressed set against a
set uploaded from the compressed text (K1 cannot tell them apart)."""
import itertools

import numpy as np
import pytest

from metamaps_amd import capi

pytestmark = pytest.mark.gpu


def hpc(s: bytes):
    """(compressed bytes, raw position of the first base of every run, of the last)"""
    out, first, last, at = bytearray(), [], [], 0
    for ch, grp in itertools.groupby(s.upper()):
        n = len(list(grp))
        out.append(ch); first.append(at); last.append(at + n - 1)
        at += n
    return bytes(out), np.array(first, dtype=np.int64), np.array(last, dtype=np.int64)


def dup30(rng, s: np.ndarray) -> np.ndarray:
    """30 % of the positions duplicated"""
    return np.repeat(s, 1 + (rng.random(len(s)) < 0.3))


def sequences():
    rng = np.random.default_rng(11)
    rnd = lambda n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    alt = lambda n: bytes(b"AC"[j & 1] for j in range(n))
    S = [rnd(n) for n in (0, 1, 15, 16, 17, 31, 32, 33)]
    S += [b"A" * 16, b"T" * 33, alt(16), alt(33)]
    S += [b"AC" * 5 + b"G" * k + b"T" + b"ACGT" * 5 for k in (5, 6, 7)]          # a run that ends at base 15, 16, 17 of a word
    S += [b"ACG" + b"T" * 45 + b"GCA"]                                           # a run spanning three words
    S += [b"", rnd(70), b"", b"", rnd(40)]                                       # empty sequences between non-empty ones
    S += [b"G" * 5000]                                                           # crosses wave and workgroup tiles
    S += [b"NNNNN" + rnd(30), rnd(30) + b"NNNN", rnd(13) + b"NNNNNN" + rnd(20), b"N" * 100, b"N" * 16, b"N"]   # N runs: start, end, across a word boundary, whole sequence
    S += [b"NNRRNN", b"ACNNRRNNAC", b"aAaA", b"acgtNNnnACGTTtTt", b"AAnnNNAA", rnd(20) + b"YYYYRRRR" + b"N" * 40 + rnd(5)]
    S += [dup30(rng, np.frombuffer(rnd(300_000), dtype=np.uint8)).tobytes()]     # 300 kb random, 30 % of the positions duplicated
    S += [b"ACGT" * 8 + b"T", b"T" * 16, b"T" + b"ACGT" * 4, b"ACGN", b"NNAC"]    # neighbours that end and begin with the same base: they must not merge
    big = bytearray(dup30(rng, np.frombuffer(rnd(3000), dtype=np.uint8)).tobytes())
    big[100:104] = b"NNNN"; big[1000:1001] = b"n"; big[2000:2100] = b"K" * 100
    S += [bytes(big)]
    return S


@pytest.fixture(scope="module")
def gpu():
    ctx = capi.Context(0)
    S = sequences()
    ref = [hpc(s) for s in S]
    yield ctx, S, ref
    ctx.close()


def _check_set(C, S, ref):
    assert C.count == len(S)
    assert C.lengths().tolist() == [len(r[0]) for r in ref]
    assert C.total_bases == sum(len(r[0]) for r in ref)
    buf, ln = C.fetch_range(0, C.count)
    assert buf.tobytes() == b"".join(r[0] for r in ref)
    for i in (0, 5, 20, len(S) - 1):
        assert C.fetch(i, len(ref[i][0])) == ref[i][0]


def test_compressed_set_equals_the_definition(gpu):
    ctx, S, ref = gpu
    assert len(S) >= 40
    R = ctx.seqset(S)
    C = R.hpc()
    _check_set(C, S, ref)
    buf, _ = R.fetch_range(0, R.count)                              # the raw set is left as it was
    assert buf.tobytes() == b"".join(s.upper() for s in S)
    C.close(); R.close()


def _nt16(s: bytes, rev: bool):
    codes = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}
    comp = bytes.maketrans(b"ACGTMRWSYKVHDBN", b"TGCAKYWSRMBDHVN")
    t = s.upper()
    if rev:
        t = t.translate(comp)[::-1]                                 # what a BAM record with flag 0x10 stores
    v = [codes[c] for c in t] + [0]
    return bytes((v[2 * j] << 4) | v[2 * j + 1] for j in range((len(t) + 1) // 2)), len(t), rev


def test_compressed_set_from_nt16_staging(gpu):
    ctx, S, ref = gpu
    R = ctx.seqset_nt16([_nt16(s, bool(i & 1)) for i, s in enumerate(S)])
    C = R.hpc()
    _check_set(C, S, ref)
    C.close(); R.close()


def test_map_to_raw_everywhere(gpu):
    ctx, S, ref = gpu
    R = ctx.seqset(S)
    C, M = R.hpc(want_map=True)
    raw_len, c_len = M.lengths()
    assert raw_len.tolist() == [len(s) for s in S] and c_len.tolist() == [len(r[0]) for r in ref]
    seq = np.concatenate([np.full(len(r[0]) + 100, i, dtype=np.int32) for i, r in enumerate(ref)])
    pos = np.concatenate([np.arange(len(r[0]) + 100, dtype=np.int64) for r in ref])
    want_first = np.concatenate([np.concatenate([r[1], len(s) + np.arange(100, dtype=np.int64)]) for s, r in zip(S, ref)])
    want_last = np.concatenate([np.concatenate([r[2], len(s) + np.arange(100, dtype=np.int64)]) for s, r in zip(S, ref)])
    first, last = M.to_raw(seq, pos)
    assert np.array_equal(first, want_first)
    assert np.array_equal(last, want_last)
    total_raw = sum(len(s) for s in S)
    assert 0 < M.device_bytes < 0.25 * total_raw + 64 * len(S) + 4096   # less than the packed raw set (plus per-sequence bookkeeping)
    M.close(); C.close(); R.close()


def test_minimizers_cannot_tell_the_layouts_apart(gpu):
    ctx, S, ref = gpu
    R = ctx.seqset(S)
    C = R.hpc()
    T = ctx.seqset([r[0] for r in ref])                             # uploaded from the compressed text
    for k, w in ((16, 10), (11, 5)):
        a = ctx.minimizers(C, k, w)
        b = ctx.minimizers(T, k, w)
        assert len(a[1]) > 1000
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    T.close(); C.close(); R.close()


def test_records_to_raw(gpu):
    """mm_mapping_to_raw: mapping on compressed sequences, records translated on the device == the definition applied to the fetched records"""
    ctx, _, _ = gpu
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    contigs = [dup30(rng, acgt[rng.integers(0, 4, 40_000)]).tobytes() for _ in range(3)]
    reads = []
    for j in range(40):
        c = contigs[j % 3]
        a = int(rng.integers(0, len(c) - 4000))
        reads.append(c[a:a + 4000])
    R, Q = ctx.seqset(contigs), ctx.seqset(reads)
    RC, M = R.hpc(want_map=True)
    QC = Q.hpc()
    k, w = 16, 5
    idx = ctx.index(RC, k, w)
    mp = ctx.map_batch(idx, QC, k, w, min_read_len=500)
    mp.add_qualities(k)
    off, before = mp.fetch()
    before = before.copy()
    assert len(before) >= 40
    end = mp.to_raw(M)
    _, after = mp.fetch()
    qlen = QC.lengths()
    cref = [hpc(c) for c in contigs]
    for i in range(len(before)):
        c, s = int(before["ref_contig"][i]), int(before["ref_start"][i])
        e = s + int(qlen[before["read"][i]]) - 1
        first, last, cl = cref[c][1], cref[c][2], len(cref[c][0])
        want_s = int(first[s]) if s < cl else len(contigs[c]) + s - cl
        want_e = int(last[e]) if e < cl else len(contigs[c]) + e - cl
        assert (int(after["ref_start"][i]), int(end[i])) == (want_s, want_e), i
    for f in ("read", "ref_contig", "shared", "sketch", "strand", "mapq"):
        assert np.array_equal(before[f], after[f])
    for o in (mp, idx, QC, RC, M, Q, R):
        o.close()
