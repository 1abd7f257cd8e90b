"""Reads with an exact amount of work, for the tests that walk the size-class edges of the per-read kernels (test_gpu_size_classes.py).

The per-read kernels are picked from a read's number of minimizers (K2), sketch hashes (K3, K5) or seed hits (K4).  A read length only
approximates these, so the reads here are found with the oracle: every read is a prefix of one sequence, the quantity is non-decreasing in the
prefix length and grows by at most one per base (the winnowing emits at most one minimizer per position, orc_core.hpp add_minimizers), and a
bisection finds the shortest prefix that reaches the count.  The result is asserted against the oracle, never assumed.  Tests only, CPU only."""
import numpy as np

_COMP = np.zeros(256, dtype=np.uint8)
_COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)

# one period of the source: random sequence, then a tandem repeat, an exact copy and a reverse-complement copy of earlier sequence
PERIOD, REPEAT_LEN = 400, 40
MIN_DUP_SHARE = 0.10                                               # of a read's minimizers share their hash with another one of the read
DUP_CHECK_FROM = 1000                                              # minimizers from which a read is held to MIN_DUP_SHARE (some periods at least)


def revcomp(a: np.ndarray) -> np.ndarray:
    return _COMP[a[::-1]]


def source_sequence(seed: int, length: int) -> bytes:
    """Random sequence in which duplicated hashes matter.  Every PERIOD bases hold, behind fresh random sequence, three repeats of REPEAT_LEN
    bases: a tandem repeat (unit of 3-23 bases), an exact copy of a stretch some kb back (same hashes, same strand) and the reverse complement
    of another such stretch (same hashes, other strand: an inverted repeat).  Made period by period from one generator, so a longer
    sequence of the same seed starts with the shorter one."""
    rng = np.random.default_rng(seed)
    out = np.empty((length + PERIOD - 1) // PERIOD * PERIOD, dtype=np.uint8)
    for at in range(0, len(out), PERIOD):
        fresh = PERIOD - 3 * REPEAT_LEN
        out[at:at + fresh] = BASES[rng.integers(0, 4, fresh)]
        p = at + fresh
        unit = BASES[rng.integers(0, 4, int(rng.integers(3, 24)))]
        out[p:p + REPEAT_LEN] = np.tile(unit, REPEAT_LEN // len(unit) + 1)[:REPEAT_LEN]
        p += REPEAT_LEN
        for inverted in (False, True):
            lo = max(0, at - 4000)                                 # up to 4 kb back; inside this period's fresh part at the start
            src = int(rng.integers(lo, at + fresh - 2 * REPEAT_LEN))
            piece = out[src:src + REPEAT_LEN]
            out[p:p + REPEAT_LEN] = revcomp(piece) if inverted else piece
            p += REPEAT_LEN
    return out[:length].tobytes()


def duplicate_profile(h: np.ndarray, st: np.ndarray):
    """(share of the minimizers whose hash another minimizer of the read has too, number of hashes that occur on both strands)"""
    if len(h) == 0:
        return 0.0, 0
    order = np.argsort(h, kind="stable")
    hs, ss = h[order], st[order]
    first = np.concatenate(([True], hs[1:] != hs[:-1]))
    run = np.cumsum(first) - 1
    size = np.bincount(run)
    plus = np.bincount(run, weights=(ss > 0))
    mixed = int(np.sum((plus > 0) & (plus < size)))
    return float(np.sum(size[size > 1])) / len(h), mixed


def sketch_of(h: np.ndarray, st: np.ndarray):
    """the sketch a stable sort by hash gives: (distinct hashes ascending, strand of the first minimizer of every run in winnowing order,
    True where all minimizers of the run have that strand)"""
    order = np.argsort(h, kind="stable")
    hs, ss = h[order], st[order]
    first = np.concatenate(([True], hs[1:] != hs[:-1])) if len(hs) else np.zeros(0, dtype=bool)
    run = np.cumsum(first) - 1
    size = np.bincount(run) if len(hs) else np.zeros(0, dtype=np.int64)
    plus = np.bincount(run, weights=(ss > 0)) if len(hs) else np.zeros(0)
    return hs[first], ss[first], (plus == 0) | (plus == size)


def _shortest_prefix(count_of, seq: bytes, target: int, lo: int, what: str) -> int:
    """smallest L in [lo, len(seq)] with count_of(seq[:L]) >= target, which must then be exactly target"""
    hi = len(seq)
    if count_of(seq[:hi]) < target:
        raise ValueError(f"the whole sequence of {hi} bases has fewer than {target} {what}")
    while lo < hi:
        mid = (lo + hi) // 2
        if count_of(seq[:mid]) >= target:
            hi = mid
        else:
            lo = mid + 1
    got = count_of(seq[:lo])
    if got != target:
        raise ValueError(f"no prefix has exactly {target} {what}: {lo} bases have {got}, one base fewer has less than {target}")
    return lo


def _ladder(count_of, seq: bytes, counts, lo: int, what: str):
    """one prefix per entry of counts, in the order of counts; the bisection of a count starts at the prefix of the next smaller one"""
    length = {}
    at = lo
    for c in sorted(set(int(c) for c in counts)):
        at = length[c] = _shortest_prefix(count_of, seq, c, at, what)
    return [seq[:length[int(c)]] for c in counts]


def _reads_from_source(oracle, k, w, counts, seed, count_of, what):
    need = max(int(c) for c in counts)
    length = max(PERIOD, (need * (w + 1) // 2 * 5 // 4 + k + w + PERIOD) // PERIOD * PERIOD)
    while True:
        src = source_sequence(seed, length)
        if count_of(src) >= need:
            break
        length *= 2
    lo = max(k, w) - 1                                            # the longest read without any minimizer
    reads = _ladder(count_of, src, counts, lo, what)
    for c, q in zip(counts, reads):
        h, _, st = oracle.minimizers(q, k, w)
        assert count_of(q) == c, (what, c, len(q))
        if len(h) >= DUP_CHECK_FROM:
            share, mixed = duplicate_profile(h, st)
            assert share >= MIN_DUP_SHARE, (what, c, share)
            assert mixed >= 2, (what, c, mixed)                   # hashes whose minimizers lie on both strands
    return reads


def reads_with_minimizers(oracle, k: int, w: int, counts, seed: int):
    """one read per entry of counts, each a prefix of source_sequence(seed, ...), with exactly that many minimizers by the oracle.  Reads of
    DUP_CHECK_FROM minimizers or more are asserted to have MIN_DUP_SHARE of them in runs of equal hashes, and runs that mix both strands."""
    return _reads_from_source(oracle, k, w, counts, seed, lambda q: len(oracle.minimizers(q, k, w)[0]), "minimizers")


def reads_with_sketch_size(oracle, k: int, w: int, sizes, seed: int):
    """the same for the sketch size: the number of distinct minimizer hashes of the read"""
    return _reads_from_source(oracle, k, w, sizes, seed, lambda q: len(np.unique(oracle.minimizers(q, k, w)[0])), "distinct minimizer hashes")


def reads_with_hits(oracle_index, contig: bytes, k: int, w: int, counts, pi: float = 80.0):
    """one read per entry of counts, each a prefix of `contig` (a stretch of one reference contig of oracle_index), with exactly that many
    raw seed hits by the oracle's map_read.  A mostly unique contig adds one hit per sketch hash; where a hash with several occurrences
    steps over a count, ValueError."""
    def hits(q):
        if len(q) < max(k, w) or len(oracle_index.o.minimizers(q, k, w)[0]) == 0:
            return 0
        return len(oracle_index.map_read(q, pi)["hit_contig"])
    reads = _ladder(hits, contig, counts, max(k, w) - 1, "seed hits")
    for c, q in zip(counts, reads):
        assert hits(q) == c, (c, len(q))
    return reads


def write_fasta(path: str, contigs, prefix: str = "c"):
    with open(path, "wb") as f:
        for i, s in enumerate(contigs):
            f.write(b">" + f"{prefix}{i}".encode() + b"\n")
            for a in range(0, len(s), 80):
                f.write(s[a:a + 80] + b"\n")


def substituted(seq: bytes, rate: float, seed: int) -> bytes:
    """seq with `rate` of its bases replaced by another base: a diverged copy at the same coordinates"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    at = np.flatnonzero(rng.random(len(a)) < rate)
    code = np.searchsorted(BASES, a[at])
    a[at] = BASES[(code + rng.integers(1, 4, len(at))) % 4]
    return a.tobytes()


def random_contig(seed: int, length: int) -> bytes:
    return BASES[np.random.default_rng(seed).integers(0, 4, length)].tobytes()


def border_pairs(h: np.ndarray, st: np.ndarray, ipt: int):
    """The LDS sort leaves thread t with the sorted positions t * ipt .. t * ipt + ipt - 1, and the unique and ambiguity pass reads the
    last element of thread t - 1 through shared memory.  (neighbours in the stably sorted order that lie across such a border and have one
    hash, those of them that differ in strand): the pairs for which that hand-over decides the result"""
    order = np.argsort(h, kind="stable")
    hs, ss = h[order], st[order]
    at = np.arange(ipt, len(hs), ipt)
    same = hs[at] == hs[at - 1]
    return int(same.sum()), int((same & (ss[at] != ss[at - 1])).sum())


# ---- the ladders of test_gpu_size_classes.py: fixed lists, derived from the IPT lists of csrc/mm_size_classes.hpp

K2_IPTS = [4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64]
K4_IPTS = [1, 2, 3, 4, 6, 8, 12, 16]


def _edges(ipts, extra):
    out = []
    for c in list(extra) + [256 * ipt + d for ipt in ipts for d in (-1, 0, 1)]:
        if c not in out:
            out.append(c)
    return sorted(out)


def lds_ipt(ipts, count):
    """elements per thread of the LDS sort that takes `count` elements: the smallest of ipts with 256 * IPT >= count; None beyond the last"""
    return next((ipt for ipt in ipts if 256 * ipt >= count), None)


K2_COUNTS = _edges(K2_IPTS, [0, 1, 2, 255, 256, 257, 16386])           # 16 383 / 16 384 / 16 385 are the edges of IPT = 64
K2_ALONE = [16383, 16384, 16385]                                        # run again as single-read batches
K4_COUNTS = _edges(K4_IPTS, [0, 1, 2, 4098])                            # 4 095 / 4 096 / 4 097 are the edges of IPT = 16
K1_POSITIONS = [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
K1_KW = [(15, 1), (15, 2), (15, 8), (16, 1), (16, 2), (16, 8)]
SF_SMAX = 2816
K3_FAR = [300, 1000, 5000, 9000]                                        # reads far below and far above the edge, in its batch
K3_SIZES = sorted(K3_FAR + [SF_SMAX - 1, SF_SMAX, SF_SMAX + 1])
L2_SKETCH_LIMIT = 32768
K5_DENSE_FROM = 13000
K5_CLASS_EDGES = [3072, 7168, 16384]
K5_SIZES = [t + d for t in K5_CLASS_EDGES + [K5_DENSE_FROM, L2_SKETCH_LIMIT] for d in (-1, 0, 1)]
K5_SMALL_DENSE_FROM = 1500
K5_SMALL_SIZES = [K5_SMALL_DENSE_FROM - 1, K5_SMALL_DENSE_FROM, K5_SMALL_DENSE_FROM + 1]
K5_LDS_SIZES = [s for s in K5_SIZES if s >= K5_DENSE_FROM - 1]          # with the dense path switched off below the limit: classes D and C

K2_KW, K2_SEED = (16, 2), 41
K4_KW = (16, 2)
L2_KW, L2_SEED = (16, 1), 43                                            # K3 and K5
FLANK = 5000
SRC_CONTIG = 1                                                          # of world_contigs: holds the source of the K3 and K5 reads
K4_CONTIG, K4_AT, K4_LEN = 0, 7001, 9000                                # the stretch the K4 reads are prefixes of
K4_COPY, K4_COPY_CONTIG = (40, 100), 5                                  # bases of that stretch that contig 5 holds too
REJECTED_CONTIG = 6                                                     # the copy of the source that L2 rejects


def world_contigs(source_seed):
    """the reference of the mapping tests: a random contig; one that holds 50 kb of the reads' source between random flanks; three diverged
    copies of that one (3 %, 8 % and reverse-complemented, 18 % of the bases substituted), so that a read has candidates on several contigs and
    on both strands, with different numbers of shared hashes; a random contig with a copy of 60 bases near the start of the K4 stretch, so
    that the hit lists of the K4 reads hold two contigs (two hits per hash there, which is why the copy is short and ends before the
    ladder's count of 255); and a copy with 19 % substituted, which at k = 16 still passes L1 and lies below the identity threshold of
    80 %: the candidate that L2 rejects"""
    home = random_contig(104, FLANK) + source_sequence(source_seed, 50_000) + random_contig(105, FLANK)
    rc = revcomp(np.frombuffer(substituted(home, 0.08, 107), dtype=np.uint8)).tobytes()
    first = random_contig(101, 50_000)
    a, b = K4_AT + K4_COPY[0], K4_AT + K4_COPY[1]
    return [first, home, substituted(home, 0.03, 106), rc, substituted(home, 0.18, 108)[2000:-3000],
            random_contig(109, 20_000) + first[a:b] + random_contig(110, 20_000), substituted(home, 0.19, 200)[2000:-3000]]


def k4_stretch(contigs):
    return contigs[K4_CONTIG][K4_AT:K4_AT + K4_LEN]                     # of a random contig: mostly one hit per sketch hash


def shuffled(n, seed):
    return np.random.default_rng(seed).permutation(n)
