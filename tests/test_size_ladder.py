"""tests/size_ladder.py on the CPU: the builder meets every count of the ladders of test_gpu_size_classes.py exactly, its source sequence makes
duplicated hashes matter (at least a tenth of a long read's minimizers share their hash with another one, some runs mix both strands), and the
same seed gives the same bytes."""
import numpy as np
import pytest

import size_ladder as sl


def test_source_sequence_is_seeded_and_extends_itself():
    a, b = sl.source_sequence(5, 30_000), sl.source_sequence(5, 30_000)
    assert a == b and len(a) == 30_000 and set(a) <= set(b"ACGT")
    assert sl.source_sequence(5, 47_123).startswith(a) and sl.source_sequence(6, 30_000) != a
    # the three kinds of repeat are there: an exact copy and a reverse-complement copy of earlier sequence, and a tandem repeat, in every period
    arr = np.frombuffer(a, dtype=np.uint8)
    for at in range(0, 30_000, sl.PERIOD):
        p = at + sl.PERIOD - 3 * sl.REPEAT_LEN
        tandem, exact, inverted = (a[p + i * sl.REPEAT_LEN:p + (i + 1) * sl.REPEAT_LEN] for i in range(3))
        assert any(tandem == (tandem[:u] * sl.REPEAT_LEN)[:sl.REPEAT_LEN] for u in range(3, 24)), at
        assert a.find(exact) < p + sl.REPEAT_LEN, at
        assert a.find(sl.revcomp(np.frombuffer(inverted, dtype=np.uint8)).tobytes()) < p, at
    assert len(arr) == 30_000


def test_k2_ladder_counts_and_duplicates(oracle_lib):
    k, w = sl.K2_KW
    assert sl.K2_COUNTS[:6] == [0, 1, 2, 255, 256, 257] and sl.K2_COUNTS[-4:] == [16383, 16384, 16385, 16386]
    assert all(256 * ipt + d in sl.K2_COUNTS for ipt in sl.K2_IPTS for d in (-1, 0, 1))
    reads = sl.reads_with_minimizers(oracle_lib, k, w, sl.K2_COUNTS, sl.K2_SEED)
    assert reads == sl.reads_with_minimizers(oracle_lib, k, w, sl.K2_COUNTS, sl.K2_SEED)
    n_mixed_reads = 0
    for c, q in zip(sl.K2_COUNTS, reads):
        h, _, st = oracle_lib.minimizers(q, k, w)
        assert len(h) == c and reads[-1].startswith(q)
        share, mixed = sl.duplicate_profile(h, st)
        if c >= sl.DUP_CHECK_FROM:
            assert share >= sl.MIN_DUP_SHARE and mixed >= 2, (c, share, mixed)
        n_mixed_reads += mixed > 0
        eh, es, pure = sl.sketch_of(h, st)
        assert np.array_equal(eh, np.unique(h)) and int((~pure).sum()) == mixed
        # the hand-over of the last element between neighbouring threads of the LDS sort decides something in every read of a class: a run
        # of equal hashes lies across a thread border, and so does a pair of them that differs in strand
        ipt = sl.lds_ipt(sl.K2_IPTS, c)
        if ipt is not None and c >= 255:
            same, differ = sl.border_pairs(h, st, ipt)
            assert same >= 1 and differ >= 1, (c, ipt, same, differ)
    assert n_mixed_reads >= 10
    assert max(len(q) for q in reads) < 30_000                    # 16 386 minimizers at w = 2: ~25 kb
    shuffled = [sl.K2_COUNTS[i] for i in sl.shuffled(len(sl.K2_COUNTS), 11)]
    assert sl.reads_with_minimizers(oracle_lib, k, w, shuffled, sl.K2_SEED) == [reads[sl.K2_COUNTS.index(c)] for c in shuffled]


def test_sketch_size_ladder(oracle_lib):
    k, w = sl.L2_KW
    sizes = sorted(set(sl.K3_SIZES + sl.K5_SIZES + sl.K5_SMALL_SIZES))
    for t in (sl.SF_SMAX, 3072, 7168, 13000, 16384, 32768, sl.K5_SMALL_DENSE_FROM):
        assert all(t + d in sizes for d in (-1, 0, 1))
    reads = sl.reads_with_sketch_size(oracle_lib, k, w, sizes, sl.L2_SEED)
    src = sl.world_contigs(sl.L2_SEED)[sl.SRC_CONTIG][sl.FLANK:-sl.FLANK]
    for s, q in zip(sizes, reads):
        assert len(np.unique(oracle_lib.minimizers(q, k, w)[0])) == s and src.startswith(q)
    assert max(len(q) for q in reads) < 45_000


def test_hit_ladder(oracle_lib, tmp_path):
    k, w = sl.K4_KW
    assert sl.K4_COUNTS[:3] == [0, 1, 2] and sl.K4_COUNTS[-4:] == [4095, 4096, 4097, 4098]
    assert all(256 * ipt + d in sl.K4_COUNTS for ipt in sl.K4_IPTS for d in (-1, 0, 1))
    contigs = sl.world_contigs(sl.K2_SEED)
    assert all(40_000 <= len(c) <= 60_000 for c in contigs) and len(contigs) == 7
    fasta = str(tmp_path / "ref.fa")
    sl.write_fasta(fasta, contigs)
    oi = oracle_lib.index(fasta, k, w)
    reads = sl.reads_with_hits(oi, sl.k4_stretch(contigs), k, w, sl.K4_COUNTS, 80.0)
    for c, q in zip(sl.K4_COUNTS, reads):
        n = len(oi.map_read(q, 80.0)["hit_contig"]) if len(q) >= max(k, w) else 0
        assert n == c and contigs[sl.K4_CONTIG].find(q) == sl.K4_AT
    # a count that a hash with several occurrences steps over is refused, not approximated
    twice = sl.random_contig(9, 400)
    sl.write_fasta(fasta, [twice + sl.random_contig(10, 300) + twice])
    oj = oracle_lib.index(fasta, k, w)
    per_len = [len(oj.map_read(twice[:n], 80.0)["hit_contig"]) for n in range(k + w, 60)]
    missing = next(c for c in range(1, max(per_len)) if c not in per_len)
    with pytest.raises(ValueError):
        sl.reads_with_hits(oj, twice, k, w, [missing], 80.0)
    oi.close(); oj.close()
