"""Inputs at the structural edges of the index build, chosen on the CPU.  Seeded generators, nothing stored: every world states, as
predicates on its model (index_model.build), the condition it exists for.  Two facts make the constructions work: the entries of a
prefix are a prefix of the whole contig's entries and grow by 0 or 1 per base (so any entry count is reachable by bisecting the prefix
length), and a homopolymer yields a single entry (so same-hash chains need tandem copies of a unit)."""
import random
from types import SimpleNamespace

import numpy as np

import index_model as im

K, W = 16, 8
TILE = 2048
LIST_LENGTHS = (7, 8, 9, 15, 16, 17, 4095, 4096, 4097)
HIST_BINS = 4096


def rand_seq(rnd, n, alphabet=b"ACGT"):
    return bytes(rnd.choice(alphabet) for _ in range(n))


class World:
    def __init__(self, name, contigs, oracle, kws=((K, W),), conditions=(), reads=()):
        self.name, self.contigs, self.oracle, self.kws = name, list(contigs), oracle, tuple(kws)
        self.conditions = list(conditions)                          # (what, (k, w), predicate on the model)
        self.units = list(reads)                                    # sequences worth mapping against it
        self._models = {}

    def model(self, k=K, w=W):
        if (k, w) not in self._models:
            self._models[(k, w)] = im.build(self.contigs, k, w, self.oracle)
        return self._models[(k, w)]

    def failed_conditions(self):
        return [what for what, kw, pred in self.conditions if not pred(self.model(*kw))]


def _count(oracle, seq, k=K, w=W):
    return len(oracle.minimizers(seq, k, w)[0]) if len(seq) - k + 1 >= w else 0


def prefix_with_entries(oracle, seq, n, k=K, w=W):
    """the shortest prefix of seq with n entries"""
    assert _count(oracle, seq, k, w) >= n
    lo, hi = 0, len(seq)
    while lo < hi:
        mid = (lo + hi) // 2
        if _count(oracle, seq[:mid], k, w) < n:
            lo = mid + 1
        else:
            hi = mid
    assert _count(oracle, seq[:lo], k, w) == n
    return seq[:lo]


def _cond(what, pred, kw=(K, W)):
    return (what, kw, pred)


def tile_contig(oracle, n, seed=11):
    return prefix_with_entries(oracle, rand_seq(random.Random(seed), 24_000), n)


def none(oracle):
    return World("none", [], oracle, conditions=[_cond("no contigs, no entries", lambda m: m.C == 0 and m.N == 0 and m.U == 0)])


def meta_only(oracle):
    rnd = random.Random(21)
    return World("meta_only", [b"", b"ACGT", rand_seq(rnd, 22)], oracle,
                 conditions=[_cond("three contigs, no entries", lambda m: m.C == 3 and m.N == 0 and int(m.dir_off[-1]) == 6)])


def one(oracle):
    return World("one", [rand_seq(random.Random(22), 23)], oracle, conditions=[_cond("a single entry", lambda m: m.N == 1 and m.U == 1 and m.P == 8)])


def tile_N(oracle):
    out = []
    for n in (2047, 2048, 2049, 4096, 4097):
        out.append(World(f"tile_N[{n}]", [tile_contig(oracle, n)], oracle, conditions=[_cond(f"N == {n}", lambda m, n=n: m.N == n and m.C == 1)]))
    first = tile_contig(oracle, TILE)
    second = prefix_with_entries(oracle, rand_seq(random.Random(12), 12_000), TILE)
    for n, tail in ((2048, rand_seq(random.Random(13), 10)), (4096, second)):
        out.append(World(f"tile_N[2048+{n - TILE}]", [first, tail], oracle,
                         conditions=[_cond(f"N == {n}, the first contig ends on the tile edge", lambda m, n=n: m.N == n and m.C == 2 and int(m.cstart[1]) == TILE)]))
    return out


def _lists_contigs(seed):
    rnd = random.Random(seed)
    units = [rand_seq(rnd, 120) for _ in LIST_LENGTHS]
    contigs = []
    for u, c in zip(units, LIST_LENGTHS):
        contigs += [rand_seq(rnd, rnd.randint(0, 11)) + u + rand_seq(rnd, rnd.randint(0, 11)) for _ in range(c)]
    chain = rand_seq(rnd, 120)
    contigs.append(chain * 5)
    contigs += [rand_seq(rnd, n) for n in (0, 4, 22, 23, 511, 512, 513, 1023, 1024, 1025)]
    rnd.shuffle(contigs)
    shift = im.dir_shift_for(W)
    if sum((len(c) >> shift) + 2 for c in contigs) % 2 == 0:        # an odd directory: its bytes end in half a word (the checksum's tail path)
        contigs.append(rand_seq(rnd, 600))
    return contigs, units + [chain]


def _edge_keys(m):
    """(equal, different): hash-sorted tile boundaries with the same key on both sides / with a head on the boundary"""
    at = np.arange(TILE, m.N, TILE)
    same = m.sorted_hash[at - 1] == m.sorted_hash[at]
    return int(same.sum()), int((~same).sum())


def lists(oracle):
    conds = [_cond(f"lists of {c} entries", lambda m, c=c: m.hist.get(c, 0) > 0) for c in LIST_LENGTHS]
    conds += [_cond("a hash run straddles a tile edge", lambda m: _edge_keys(m)[0] > 0), _cond("a head sits on a tile edge", lambda m: _edge_keys(m)[1] > 0),
              _cond("lists at and beyond the histogram's bins", lambda m: max(m.hist) >= HIST_BINS and m.hist.get(HIST_BINS - 1, 0) > 0),
              _cond("metadata-only and empty contigs between real ones", lambda m: bool(np.any((np.diff(m.cstart.astype(np.int64)) == 0)[1:-1]))),
              _cond("an odd number of directory elements", lambda m: int(m.dir_off[-1]) % 2 == 1),
              _cond("contig lengths on either side of a directory bucket", lambda m: {511, 512, 513, 1023, 1024, 1025} <= set(m.contig_len.tolist()))]
    for seed in range(31, 39):                                      # the tile-edge conditions depend on where the hashes fall: take the first seed that has both
        contigs, units = _lists_contigs(seed)
        wd = World("lists", contigs, oracle, conditions=conds, reads=units)
        if not wd.failed_conditions():
            break
    return wd


def tandem(oracle):
    rnd = random.Random(41)
    unit = rand_seq(rnd, 150)
    contigs = [rand_seq(rnd, 5000), unit * 70, rand_seq(rnd, 3300), unit * 200, rand_seq(rnd, 7000)]
    ALL = np.uint64(2**64 - 1)

    def both(m):
        return bool(np.any((m.pw & 6) == 6))

    def straddle(m):
        return bool(np.any((m.wpos[m.pair_first] >> m.dir_shift) != (m.wpos[m.pair_second] >> m.dir_shift)))
    return World("tandem", contigs, oracle, reads=[unit * 8],
                 conditions=[_cond("entries with both flags", both), _cond("a bitmap word of all ones", lambda m: bool(np.any(m.dup_bits == ALL))),
                             _cond("flagged entries at bit 0 and bit 63", lambda m: bool(np.any(m.dup_bits & np.uint64(1))) and bool(np.any(m.dup_bits >> np.uint64(63)))),
                             _cond("a pair across a directory bucket", straddle),
                             _cond("one hash in two contigs: neighbours in a list that are no pair", lambda m: m.n_dup < m.N - m.U)])


def wrap(oracle):
    for seed in range(400):                                          # a probe cluster that runs past the last slot of the 64-bucket table
        wd = World("wrap", [rand_seq(random.Random(1000 + seed), 640)], oracle)
        m = wd.model()
        if m.tab_buckets == 64 and m.wrapped:
            break
    wd.seed = seed
    wd.conditions = [_cond("64 buckets and a probe sequence that wraps to slot 0", lambda m: m.tab_buckets == 64 and m.wrapped and m.longest_probe >= 1)]
    return wd


def kw(oracle):
    rnd = random.Random(51)
    contigs = [tile_contig(oracle, 2049), rand_seq(rnd, 30_000), rand_seq(rnd, 20_000, b"AC")]
    return World("kw", contigs, oracle, kws=((16, 8), (16, 1), (5, 3), (21, 11), (8, 100)),
                 conditions=[_cond("few hashes, long lists", lambda m: m.U < 1024 and int(m.ucount.max()) > 64, (5, 3))])


_cache = {}


def all_worlds(oracle):
    """every world once per process (the models are cached inside)"""
    if "all" not in _cache:
        _cache["all"] = [none(oracle), meta_only(oracle), one(oracle)] + tile_N(oracle) + [lists(oracle), tandem(oracle), wrap(oracle), kw(oracle)]
    return _cache["all"]


def by_name(oracle, name):
    return next(wd for wd in all_worlds(oracle) if wd.name == name)


def read_set(world, seed=61, n_cuts=50, cut=3000, sub_rate=0.03):
    """the world's units, a few whole contigs and random cuts with substitutions (a read as long as its contig maps nowhere, so a cut
    takes at most half of it)"""
    rnd = random.Random(seed)
    real = [c for c in world.contigs if len(c) >= 120]
    reads = list(world.units) + real[:4]
    for _ in range(n_cuts if real else 0):
        c = rnd.choice(real)
        n = min(cut, len(c) // 2)
        a = rnd.randint(0, len(c) - n)
        s = bytearray(c[a:a + n])
        for i in range(n):
            if rnd.random() < sub_rate:
                s[i] = rnd.choice(b"ACGT")
        reads.append(bytes(s))
    return reads


def summary_row(world, k, w):
    m = world.model(k, w)
    return SimpleNamespace(name=world.name, k=k, w=w, N=m.N, U=m.U, P=m.P, longest_probe=m.longest_probe, wrapped=m.wrapped, buckets=m.tab_buckets)
