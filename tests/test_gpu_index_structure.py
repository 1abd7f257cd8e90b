"""The index build's hash side and the index file format, held against the host model (index_model.py) on the edge inputs of
index_worlds.py.  Everything goes through the C ABI as it is; the saved file is the tap.  Every comparison is exact."""
import random

import numpy as np
import pytest

import index_model as im
import index_worlds as iw

pytestmark = pytest.mark.gpu

WORLD_NAMES = ["none", "meta_only", "one", "tile_N[2047]", "tile_N[2048]", "tile_N[2049]", "tile_N[4096]", "tile_N[4097]", "tile_N[2048+0]",
               "tile_N[2048+2048]", "lists", "tandem", "wrap", "kw"]
DEFINED = ("pos", "cstart", "occ", "occ16", "dir", "dir_off", "dup_bits", "dup_rank", "dup_dist")     # every array but the table


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _same_taps(idx, m):
    info = idx.info()
    assert (info["n_contigs"], info["n_entries"], info["n_unique_hashes"], info["n_dup_flagged"]) == (m.C, m.N, m.U, m.n_dup)
    h, c, wp, st = idx.entries()
    assert np.array_equal(h, m.hash) and np.array_equal(c, m.contig) and np.array_equal(wp, m.wpos) and np.array_equal(st, m.strand)
    pd, nd = idx.dup_neighbours()
    assert np.array_equal(pd, m.prev_dist) and np.array_equal(nd, m.next_dist)
    hk, hn = idx.freq_hist()
    mk, mn = im.hist_arrays(m)
    assert np.array_equal(hk, mk) and np.array_equal(hn, mn)


def _defined(parsed, m):
    """the bytes of every array but the table over the range the build defines"""
    n = {"pos": m.N, "cstart": m.C + 1, "occ": m.P, "occ16": m.P, "dir": int(m.dir_off[-1]), "dir_off": m.C + 1, "dup_bits": len(m.dup_bits),
         "dup_rank": len(m.dup_rank), "dup_dist": m.n_flagged}
    return {name: parsed["arrays"][name].data[:n[name]].tobytes() for name in DEFINED}


def _build_and_audit(ctx, wd, k, w, path):
    S = ctx.seqset(wd.contigs)
    idx = ctx.index(S, k, w)
    idx.save(path)
    m = wd.model(k, w)
    p = im.parse(path)
    assert im.audit(p, m) == []
    _same_taps(idx, m)
    return S, idx, p


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_built_index_is_the_model(ctx, oracle_lib, tmp_path, name):
    wd = iw.by_name(oracle_lib, name)
    assert wd.failed_conditions() == []
    for k, w in wd.kws:
        path = str(tmp_path / "built.mmidx")
        S, idx, p = _build_and_audit(ctx, wd, k, w, path)
        m = wd.model(k, w)
        print(f"{name} k={k} w={w}: N={m.N} U={m.U} P={m.P} buckets={m.tab_buckets} longest probe={m.longest_probe} wrapped={m.wrapped}")
        if name in ("none", "meta_only", "one"):                    # ... and it loads back and maps without error
            rnd = random.Random(71)
            reads = [iw.rand_seq(rnd, 1200), iw.rand_seq(rnd, 700) + wd.contigs[-1] * 30 if wd.contigs else iw.rand_seq(rnd, 1500), b"", iw.rand_seq(rnd, 5000)]
            R = ctx.seqset(reads)
            loaded = ctx.load_index(path)
            a, b = loaded.info(), idx.info()
            if m.N == 0:                                            # (an index without entries: the loader holds one spare element where the build holds none)
                a.pop("hbm_bytes"); b.pop("hbm_bytes")
            assert a == b
            for I in (idx, loaded):
                M = ctx.map_batch(I, R, k, w)
                off, rec = M.fetch()
                if m.N == 0:
                    assert len(rec) == 0 and not off.any()
                else:
                    fasta = tmp_path / "one.fa"
                    fasta.write_bytes(b"".join(b">c%d\n%s\n" % (i, c) for i, c in enumerate(wd.contigs)))
                    oi = oracle_lib.index(str(fasta), k, w)
                    for r, q in enumerate(reads):
                        want = oi.map_read(q)["map"] if len(q) >= 1000 else np.zeros((0, 6), dtype=np.int32)
                        got = rec[off[r]:off[r + 1]]
                        assert len(got) == len(want) and np.array_equal(got["ref_start"], want[:, 1]), r
                    oi.close()
                M.close()
            loaded.close(); R.close()
        idx.close(); S.close()


@pytest.mark.parametrize("name", ["lists", "tile_N[2049]"])
def test_partitioned_sort_builds_the_same_index(ctx, oracle_lib, tmp_path, monkeypatch, name):
    """MM_INDEX_PART_MAX at N (the plain sort), N - 1, the fullest 16-bit hash prefix m (the smallest limit the build accepts) and about
    N / 7: the same index, byte for byte, but for the table's slot order; m - 1 is refused and leaves the context usable"""
    from metamaps_amd import capi
    wd = iw.by_name(oracle_lib, name)
    m = wd.model()
    top = im.top16_max(m)
    assert top >= 2
    path = str(tmp_path / "p.mmidx")
    S, idx, plain = _build_and_audit(ctx, wd, iw.K, iw.W, path)
    idx.close()
    want = _defined(plain, m)
    for part_max in (m.N, m.N - 1, top, m.N // 7):
        parts = im.partitions(m, part_max)
        print(f"{name} MM_INDEX_PART_MAX={part_max}: " + ("plain sort" if parts is None else f"{len(parts)} partitions, largest {max(parts)}"))
        assert (parts is None) == (part_max == m.N) and (parts is None or (max(parts) <= part_max and sum(parts) == m.N and len(parts) >= 2))
        monkeypatch.setenv("MM_INDEX_PART_MAX", str(part_max))
        idx = ctx.index(S, iw.K, iw.W)
        idx.save(path)
        p = im.parse(path)
        assert im.audit(p, m) == []
        got = _defined(p, m)
        for arr in DEFINED:
            assert got[arr] == want[arr], (part_max, arr)
        idx.close()
    monkeypatch.setenv("MM_INDEX_PART_MAX", str(top - 1))
    with pytest.raises(capi.MMError) as e:
        ctx.index(S, iw.K, iw.W)
    assert e.value.status == capi.MM_ERR_LIMIT
    monkeypatch.setenv("MM_INDEX_PART_MAX", str(top))
    idx = ctx.index(S, iw.K, iw.W)                                  # the next build in the same context
    idx.save(path)
    assert im.audit(im.parse(path), m) == []
    _same_taps(idx, m)
    idx.close(); S.close()


@pytest.mark.parametrize("name,max_memory,n_cuts", [("lists", 1_000_000, 50), ("tandem", 400_000, 100), ("wrap", 100_000, 150)])
def test_index_written_by_the_model_loads_and_maps_like_the_built_one(ctx, oracle_lib, tmp_path, name, max_memory, n_cuts):
    """an index file the device did not write: the loader, the checksum kernel (word and tail paths) and every consumer of the hash side
    against an independent writer.  (A cut maps once or twice: tandem, with five contigs, and wrap, whose one contig has 640 bases and whose cuts are 320, take more than 50 cuts to give 100 records.)"""
    wd = iw.by_name(oracle_lib, name)
    m = wd.model()
    S = ctx.seqset(wd.contigs)
    built = ctx.index(S, iw.K, iw.W)
    path = im.write(str(tmp_path / "model.mmidx"), m)
    loaded = ctx.load_index(path)
    assert loaded.info() == built.info()
    _same_taps(loaded, m)
    _same_taps(built, m)
    chunks = built.plan_chunks(max_memory)
    assert loaded.plan_chunks(max_memory) == chunks and (len(chunks) > 1 or name == "wrap")
    reads = iw.read_set(wd, n_cuts=n_cuts)
    R = ctx.seqset(reads)
    Mb, Ml = ctx.map_batch(built, R, iw.K, iw.W, min_read_len=50), ctx.map_batch(loaded, R, iw.K, iw.W, min_read_len=50)
    (ob, rb), (ol, rl) = Mb.fetch(), Ml.fetch()
    print(f"{name}: {len(reads)} reads, {len(rb)} records, {len(chunks)} chunks at {max_memory} bytes")
    assert np.array_equal(ob, ol) and rb.tobytes() == rl.tobytes()
    assert len(rb) > 100
    Mb.close(); Ml.close(); R.close(); loaded.close(); built.close(); S.close()


def test_damage_inside_intact_framing_is_refused_array_by_array(ctx, oracle_lib, tmp_path):
    from metamaps_amd import capi
    wd = iw.by_name(oracle_lib, "lists")
    S = ctx.seqset(wd.contigs)
    built = ctx.index(S, iw.K, iw.W)
    path = str(tmp_path / "lists.mmidx")
    built.save(path)
    p = im.parse(path)
    data = p["bytes"]

    def refused(bad, what):
        assert bad != data and len(bad) == len(data)
        open(path, "wb").write(bad)
        with pytest.raises(capi.MMError) as e:
            ctx.load_index(path)
        assert f"checksum of the {what} differs" in str(e.value), (what, str(e.value))

    for name, _, what in im.ARRAYS:
        a = p["arrays"][name]
        assert a.nbytes >= 3
        for at in (a.offset, a.offset + a.nbytes // 2, a.offset + a.nbytes - 1):
            b = bytearray(data); b[at] ^= 0x04
            refused(bytes(b), what)
    s = int(wd.model().pstart[int(np.nonzero(wd.model().ucount == 16)[0][0])])

    def swap(a):
        assert a[s] != a[s + 1]
        a[[s, s + 1]] = a[[s + 1, s]]
    refused(im.edited(p, "occ", swap, fix_sum=False), "occurrences")              # the sum depends on where a word lies
    d = p["arrays"]["dir"]
    assert d.count % 2 == 1 and d.nbytes % 8 == 4                                   # the last element lies behind the last whole word: the tail path
    b = bytearray(data)
    b[d.offset + d.nbytes - 4:d.offset + d.nbytes] = (int(d.data[-1]) + 1).to_bytes(4, "little")
    refused(bytes(b), "position directory")
    open(path, "wb").write(data)
    again = ctx.load_index(path)                                     # the undamaged bytes still load
    assert again.info() == built.info()
    again.close(); built.close(); S.close()


def test_hits_through_the_edge_lists_match_oracle(ctx, oracle_lib, tmp_path, monkeypatch):
    """the units of the lists world as reads, the frequency threshold lifted: the seed hits come out of lists of 7, 8, 9 and 4097 entries"""
    monkeypatch.setenv("MM_NO_HIT_FILTER", "1")                     # the raw seed-hit list, as test_mapping_stages_match_oracle compares it
    wd = iw.by_name(oracle_lib, "lists")
    m = wd.model()
    fasta = tmp_path / "lists.fa"
    fasta.write_bytes(b"".join(b">c%d\n%s\n" % (i, c) for i, c in enumerate(wd.contigs)))
    oi = oracle_lib.index(str(fasta), iw.K, iw.W)
    assert oi.n == m.N and oi.n_unique == m.U and oi.n_contigs == m.C
    S, R = ctx.seqset(wd.contigs), ctx.seqset(wd.units)
    idx = ctx.index(S, iw.K, iw.W)
    idx.set_freq_threshold(2**31 - 1)
    oi.set_freq_threshold(2**31 - 1)
    M = ctx.map_batch(idx, R, iw.K, iw.W, pi=80.0, min_read_len=100)
    sk_off, sk_h, _ = M.debug_sketch()
    hit_off, hit_c, hit_w = M.debug_hits()
    lengths_read = set()
    for r, q in enumerate(wd.units):
        o = oi.map_read(q, 80.0, ccap=8192)                      # (a unit lies in up to 4097 contigs)
        a, b = int(sk_off[r]), int(sk_off[r + 1])
        assert b > a and np.array_equal(sk_h[a:b], o["sketch_hash"]), r
        at = np.searchsorted(m.uh, sk_h[a:b])
        known = (at < m.U) & (m.uh[np.minimum(at, m.U - 1)] == sk_h[a:b])
        lengths_read |= set(m.ucount[at[known]].tolist())
        a, b = int(hit_off[r]), int(hit_off[r + 1])
        assert b - a == len(o["hit_contig"]) == int(m.ucount[at[known]].sum()), r
        assert np.array_equal(hit_c[a:b], o["hit_contig"]) and np.array_equal(hit_w[a:b], o["hit_wpos"]), r
    print("list lengths read:", sorted(lengths_read))
    assert {7, 8, 9, 4097} <= lengths_read
    oi.close(); M.close(); idx.close(); R.close(); S.close()
