"""The host model of the index (index_model.py) and its edge inputs (index_worlds.py), held against the oracle and against themselves:
the model's position side is the oracle's index, every world reaches the edge it was built for, a written model audits clean, and the
audit reports each single-element mutation in the array it was made in.  No GPU."""
import struct

import numpy as np
import pytest

import index_model as im
import index_worlds as iw


@pytest.fixture(scope="module")
def worlds(oracle_lib):
    return iw.all_worlds(oracle_lib)


WORLD_NAMES = ["none", "meta_only", "one", "tile_N[2047]", "tile_N[2048]", "tile_N[2049]", "tile_N[4096]", "tile_N[4097]", "tile_N[2048+0]",
               "tile_N[2048+2048]", "lists", "tandem", "wrap", "kw"]


def test_world_list_is_complete(worlds):
    assert [wd.name for wd in worlds] == WORLD_NAMES


@pytest.mark.parametrize("which", ["tandem", "kw"])
@pytest.mark.parametrize("k,w", [(16, 8), (5, 3)])
def test_model_position_side_is_the_oracles_index(oracle_lib, worlds, tmp_path, which, k, w):
    wd = iw.by_name(oracle_lib, which)
    contigs = [b"", b"ACGT"] + wd.contigs[:2] + [wd.contigs[0][:22]] + wd.contigs[2:] + [b""]    # metadata-only contigs between real ones
    fasta = tmp_path / "ref.fa"
    fasta.write_bytes(b"".join(b">c%d\n%s\n" % (i, c) for i, c in enumerate(contigs)))
    m = im.build(contigs, k, w, oracle_lib)
    oi = oracle_lib.index(str(fasta), k, w)
    oh, oc, ow, os_ = oi.dump()
    assert oi.n_contigs == m.C == len(contigs) and oi.n == m.N > 1000
    assert np.array_equal(m.hash, oh) and np.array_equal(m.contig, oc) and np.array_equal(m.wpos, ow) and np.array_equal(m.strand, os_)
    assert np.array_equal(np.diff(m.cstart.astype(np.int64)), np.bincount(oc, minlength=m.C))
    assert oi.n_unique == m.U
    cnt = np.unique(oh, return_counts=True)[1]
    hv, hc = np.unique(cnt, return_counts=True)
    assert m.hist == {int(a): int(b) for a, b in zip(hv, hc)} and sum(c * n for c, n in m.hist.items()) == m.N
    assert m.freq_threshold == oi.freq_threshold
    oi.close()


def test_model_restates_the_duplicate_definition(oracle_lib):
    """prev / next distances by the definition, entry by entry: the nearest entry of the same contig with the same hash"""
    m = iw.by_name(oracle_lib, "tandem").model()
    last, prev = {}, np.zeros(m.N, dtype=np.int32)
    for i, key in enumerate(zip(m.contig.tolist(), m.hash.tolist())):
        if key in last:
            prev[i] = i - last[key]
        last[key] = i
    nxt = np.zeros(m.N, dtype=np.int32)
    at = np.nonzero(prev)[0]
    nxt[at - prev[at]] = prev[at]
    assert np.array_equal(m.prev_dist, prev) and np.array_equal(m.next_dist, nxt) and m.n_dup == len(at) > 1000
    assert np.array_equal((m.pw & im.PW_DP) != 0, prev != 0) and np.array_equal((m.pw & im.PW_DN) != 0, nxt != 0)


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_world_reaches_its_edge(oracle_lib, worlds, name):
    wd = iw.by_name(oracle_lib, name)
    assert wd.conditions and wd.failed_conditions() == []
    for k, w in wd.kws:
        r = iw.summary_row(wd, k, w)
        print(f"{name} k={k} w={w}: N={r.N} U={r.U} P={r.P} buckets={r.buckets} longest probe={r.longest_probe} wrapped={r.wrapped}")


def test_wrap_seed_is_the_first_that_qualifies(oracle_lib, worlds):
    wd = iw.by_name(oracle_lib, "wrap")
    m = wd.model()
    print("wrap seed", wd.seed, "U", m.U, "longest probe", m.longest_probe)
    assert m.tab_buckets == 64 and int(m.tab_where.min()) == 0 and int(m.tab_where.max()) == 255


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_written_model_audits_clean(oracle_lib, worlds, tmp_path, name):
    wd = iw.by_name(oracle_lib, name)
    for k, w in wd.kws:
        m = wd.model(k, w)
        p = im.parse(im.write(str(tmp_path / "m.idx"), m))
        assert im.audit(p, m) == []
        assert p["arrays"]["occ"].count == (m.P + 2 if m.N else 1) and p["N"] == m.N


def test_array_sum_is_position_dependent_and_has_a_tail():
    a = np.arange(1, 9, dtype="<u8")
    b = a.copy(); b[[2, 5]] = b[[5, 2]]
    assert im.array_sum(a.tobytes()) != im.array_sum(b.tobytes())
    raw = a.tobytes() + b"\x01\x02\x03\x04"
    assert im.array_sum(raw) != im.array_sum(a.tobytes()) and im.array_sum(raw) != im.array_sum(raw[:-1] + b"\x05")
    # one word by hand: mix(w + C * 1)
    x = (7 + 0xD6E8FEB86659FD93) % 2**64
    x ^= x >> 31; x = x * 0x9E3779B97F4A7C15 % 2**64; x ^= x >> 29
    assert im.array_sum(struct.pack("<Q", 7)) == x


# ---- mutations: each is made in a written file (checksums recomputed unless the case is about them) ----
@pytest.fixture(scope="module")
def lists_file(oracle_lib, tmp_path_factory):
    m = iw.by_name(oracle_lib, "lists").model()
    return m, im.parse(im.write(str(tmp_path_factory.mktemp("mut") / "lists.idx"), m))


def _list_with(m, count):
    return int(np.nonzero(m.ucount == count)[0][0])


def _mut_swap_neighbours(m, p):
    s = int(m.pstart[_list_with(m, 9)])
    def f(a): a[[s + 3, s + 4]] = a[[s + 4, s + 3]]
    return im.edited(p, "occ", f), {"occ"}


def _mut_list_start(m, p):
    u = _list_with(m, 15)
    s = int(m.pstart[u])
    def shift(a): a[s + 8:m.P] = a[s:m.P - 8].copy(); a[s:s + 8] = 0
    return im.edited(im.parse(im.edited(p, "occ", shift)), "occ16", shift), {"occ", "occ16"}


def _mut_pad_nonzero(m, p):
    s = int(m.pstart[_list_with(m, 7)])
    def f(a): a[s + 7] = a[s + 6]
    return im.edited(p, "occ", f), {"occ"}


def _mut_pad_code_real(m, p):
    s = int(m.pstart[_list_with(m, 9)])
    def f(a): assert a[s + 9] >= im.HF_SLOTS; a[s + 9] = a[s + 8]
    return im.edited(p, "occ16", f), {"occ16"}


def _mut_bin_off_by_one(m, p):
    s = int(m.pstart[_list_with(m, 4097)])
    def f(a): a[s + 4096] = (int(a[s + 4096]) + 1) & 8191
    return im.edited(p, "occ16", f), {"occ16"}


def _slot_of(m, count):
    return int(m.tab_where[_list_with(m, count)])


def _mut_tab_cleared(m, p):
    s = _slot_of(m, 8)
    def f(a): a[2 * s] = 0; a[2 * s + 1] = 0
    return im.edited(p, "tab", f), {"tab"}


def _mut_tab_count(m, p):
    s = _slot_of(m, 4096)
    def f(a): a[2 * s] += np.uint64(1 << 32)
    return im.edited(p, "tab", f), {"tab"}


def _mut_tab_start(m, p):
    s = _slot_of(m, 16)
    def f(a): a[2 * s + 1] += np.uint64(8)
    return im.edited(p, "tab", f), {"tab"}


def _mut_tab_unreachable(m, p):
    s = _slot_of(m, 17)
    def f(a):
        free = np.nonzero(a[0::2] == 0)[0]
        t = int(free[free != s][len(free) // 2])
        a[2 * t], a[2 * t + 1] = a[2 * s], a[2 * s + 1]
        a[2 * s] = 0; a[2 * s + 1] = 0
    return im.edited(p, "tab", f), {"tab"}


def _mut_dir(m, p):
    def f(a): a[len(a) // 2] += 1
    return im.edited(p, "dir", f), {"dir"}


def _mut_dp_dropped(m, p):
    i = int(np.nonzero(m.pw & im.PW_DP)[0][0])
    def f(a): a[2 * i + 1] &= ~np.uint32(im.PW_DP)
    return im.edited(p, "pos", f), {"pos"}


def _mut_dup_bit(m, p):
    i = int(np.nonzero(m.pw & (im.PW_DP | im.PW_DN))[0][-1])
    def f(a): a[i >> 6] &= ~(np.uint64(1) << np.uint64(i & 63))
    return im.edited(p, "dup_bits", f), {"dup_bits"}


def _mut_dup_rank(m, p):
    def f(a): a[len(a) // 2] += np.uint64(1)
    return im.edited(p, "dup_rank", f), {"dup_rank"}


def _mut_dup_halves(m, p):
    r = int(np.nonzero((m.dup_dist >> np.uint32(16)) != (m.dup_dist & np.uint32(0xFFFF)))[0][0])
    def f(a): a[r] = (a[r] >> np.uint32(16)) | ((a[r] & np.uint32(0xFFFF)) << np.uint32(16))
    return im.edited(p, "dup_dist", f), {"dup_dist"}


def _mut_hist_row(m, p):
    buf = bytearray(p["bytes"])
    row = [int(x) for x in p["hist"][:, 0]].index(4096)
    at = p["hist_at"] + 16 * row + 8
    struct.pack_into("<q", buf, at, struct.unpack_from("<q", buf, at)[0] + 1)
    return bytes(buf), {"hist"}


def _mut_sum_words(m, p):
    s = int(m.pstart[_list_with(m, 16)])
    def f(a): assert a[s] != a[s + 1]; a[[s, s + 1]] = a[[s + 1, s]]
    return im.edited(p, "occ", f, fix_sum=False), ("occ", "checksum")


def _mut_sum_tail(m, p):
    a = p["arrays"]["dir"]
    assert a.count % 2 == 1 and a.nbytes % 8 == 4                    # the last element lies in the bytes behind the last whole word
    buf = bytearray(p["bytes"]); buf[a.offset + a.nbytes - 1] ^= 0x01
    return bytes(buf), ("dir", "checksum")


MUTATIONS = {"list_neighbours_swapped": _mut_swap_neighbours, "list_start_moved_by_8": _mut_list_start, "pad_entry_nonzero": _mut_pad_nonzero,
             "pad_code_is_a_real_bin": _mut_pad_code_real, "bin_code_off_by_one": _mut_bin_off_by_one, "table_slot_cleared": _mut_tab_cleared,
             "table_count_off_by_one": _mut_tab_count, "table_start_off_by_8": _mut_tab_start, "table_entry_behind_an_empty_slot": _mut_tab_unreachable,
             "dir_off_by_one": _mut_dir, "dp_flag_dropped": _mut_dp_dropped, "dup_bit_cleared": _mut_dup_bit, "dup_rank_off_by_one": _mut_dup_rank,
             "dup_dist_halves_exchanged": _mut_dup_halves, "hist_row_changed": _mut_hist_row, "checksum_two_words_exchanged": _mut_sum_words,
             "checksum_tail_byte_changed": _mut_sum_tail}


@pytest.mark.parametrize("case", list(MUTATIONS))
def test_audit_reports_the_mutation(lists_file, case):
    m, p = lists_file
    assert im.audit(p, m) == []
    data, want = MUTATIONS[case](m, p)
    assert data != p["bytes"]
    found = im.audit(im.parse(data), m)
    print(case, found)
    if isinstance(want, tuple):                                      # the stored sum no longer fits the bytes (the content findings come with it)
        assert any(f[0] == want[0] and f[1] == want[1] for f in found)
    else:
        assert found and {f[0] for f in found} == want
        assert not any(f[1] == "checksum" for f in found)
    if case == "table_entry_behind_an_empty_slot":
        assert any("not reachable" in str(f[2]) for f in found)
