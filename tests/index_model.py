"""What a device index is, restated in numpy from the oracle's minimizers, and a reader, a writer and an auditor of the index
file format (the comment block above IDX_VERSION in mm_index.hip).  Test infrastructure only: every comparison is exact.

build(contigs, k, w, oracle) -> Model      the definition (position side, hash side, directory, duplicates, table)
parse(path) -> dict                        the file as it is stored: header, histogram, contig table, ten arrays
write(path, model)                         a model as such a file, checksums from array_sum() below
audit(parsed, model) -> [findings]         empty when the file holds the model's index
"""
import struct
from types import SimpleNamespace

import numpy as np

PW_STRAND, PW_DP, PW_DN, PW_SHIFT = 1, 2, 4, 3
HF_BIN_SHIFT, HF_SLOTS, HF_PAD_SLOTS = 13, 8192, 64
INT_MAX = 2**31 - 1
IDX_VERSION = 3
IDX_TAIL = 0x58444E4958444E49
MAGIC = b"MMINDEX1"
SUM_C = np.uint64(0xD6E8FEB86659FD93)
MIX_C = np.uint64(0x9E3779B97F4A7C15)
U64, U32 = np.uint64, np.uint32

# the ten arrays in file order: (name, dtype, what the loader calls it in its checksum message)
ARRAYS = [("pos", "<u4", "entries"), ("cstart", "<u8", "contig starts"), ("occ", "<u8", "occurrences"), ("occ16", "<u2", "occurrence bins"),
          ("tab", "<u8", "hash table"), ("dir", "<u4", "position directory"), ("dir_off", "<u8", "directory offsets"),
          ("dup_bits", "<u8", "duplicate bits"), ("dup_rank", "<u8", "duplicate ranks"), ("dup_dist", "<u4", "duplicate distances")]
ARRAY_DTYPE = {n: d for n, d, _ in ARRAYS}
ARRAY_WHAT = {n: w for n, _, w in ARRAYS}


# ---- small restatements ---------------------------------------------------------------------------
def dir_shift_for(w: int) -> int:
    """build_directory's rule: about 128 entries per bucket at the expected density 2 / (w + 1)"""
    shift = 4
    while 128.0 * (w + 1) / 2.0 >= float(2 << shift) and shift < 20:
        shift += 1
    return shift


def tab_buckets_for(U: int) -> int:
    slots = int(float(U) / 0.55) + 4
    return max((slots + 3) // 4, 64)


def tab_slot(h, buckets: int):
    """home slot of hash h (scalar or array): first slot of a 4-slot bucket"""
    h = np.asarray(h, dtype=U64)
    m = (h * U64(0x9E3779B1)) & U64(0xFFFFFFFF)
    return (((m * U64(buckets)) >> U64(32)) << U64(2)).astype(np.int64)


def hf_pad_code(list_start, j):
    list_start, j = np.asarray(list_start, dtype=U64), np.asarray(j, dtype=U64)
    return (U64(HF_SLOTS) + (((list_start >> U64(3)) * U64(5) + j) & U64(HF_PAD_SLOTS - 1))).astype(np.uint16)


def freq_threshold(hist: dict, U: int) -> int:
    """the 0.001 % rule over the histogram (float arithmetic, truncated)"""
    thr = INT_MAX
    if U <= 0:
        return thr
    ignore = int(np.float32(U) * np.float32(0.001) / np.float32(100))
    s = 0
    for c in sorted(hist, reverse=True):
        s += hist[c]
        if s < ignore:
            thr = c
        elif s == ignore:
            thr = c
            break
        else:
            break
    return thr


def sum_mix(x):
    x = x ^ (x >> U64(31))
    x = x * MIX_C
    return x ^ (x >> U64(29))


def array_sum(raw: bytes) -> int:
    """checksum of an array's bytes: sum of mix(word + C * (i + 1)) over the 8-byte words, plus the same over the bytes of a last
    partial word, modulo 2^64"""
    nw = len(raw) >> 3
    words = np.frombuffer(raw, dtype="<u8", count=nw).astype(U64)
    acc = int(np.sum(sum_mix(words + SUM_C * np.arange(1, nw + 1, dtype=U64)), dtype=U64)) if nw else 0
    tail = np.frombuffer(raw, dtype=np.uint8, offset=nw << 3).astype(U64)
    if len(tail):
        acc += int(np.sum(sum_mix(tail + SUM_C * (U64(nw + 1) + np.arange(len(tail), dtype=U64))), dtype=U64))
    return acc & (2**64 - 1)


# ---- the definition -------------------------------------------------------------------------------
def build(contigs, k: int, w: int, oracle, dup_sat: int = 65535) -> SimpleNamespace:
    C = len(contigs)
    clen = np.array([len(c) for c in contigs], dtype=np.int64)
    hs, ws, ss = [], [], []
    counts = np.zeros(C, dtype=np.int64)
    for i, c in enumerate(contigs):
        if len(c) - k + 1 < w:                                      # no window fits: metadata only
            continue
        h, wp, st = oracle.minimizers(bytes(c), k, w)
        counts[i] = len(h)
        hs.append(h); ws.append(wp); ss.append(st)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    hash_, wpos, strand = cat(hs, U32), cat(ws, np.int64), cat(ss, np.int32)
    N = len(hash_)
    cstart = np.zeros(C + 1, dtype=U64)
    cstart[1:] = np.cumsum(counts)
    contig = np.repeat(np.arange(C, dtype=np.int64), counts)
    pw0 = ((wpos << PW_SHIFT) | (strand == 1)).astype(U32)           # no duplicate flags: what the occurrence lists carry

    # hash side: stable sort by hash keeps (contig, position) order inside a list
    order = np.argsort(hash_, kind="stable")
    sh = hash_[order]
    uh, ustart, ucount = np.unique(sh, return_index=True, return_counts=True)
    U = len(uh)
    ustart, ucount = ustart.astype(np.int64), ucount.astype(np.int64)
    pcount = (ucount + 7) & ~7
    pstart = np.zeros(U + 1, dtype=np.int64)
    pstart[1:] = np.cumsum(pcount)
    P = int(pstart[-1])
    list_of_sorted = np.repeat(np.arange(U, dtype=np.int64), ucount)
    dst = pstart[list_of_sorted] + (np.arange(N, dtype=np.int64) - ustart[list_of_sorted])
    occ = np.zeros(P, dtype=U64)
    occ[dst] = (contig[order].astype(U64) << U64(32)) | pw0[order].astype(U64)
    cbase = np.zeros(C + 1, dtype=np.int64)
    cbase[1:] = np.cumsum(clen)
    list_of_padded = np.repeat(np.arange(U, dtype=np.int64), pcount)
    occ16 = hf_pad_code(pstart[list_of_padded], np.arange(P, dtype=np.int64) - pstart[list_of_padded]) if P else np.zeros(0, dtype=np.uint16)
    occ16[dst] = (((cbase[contig[order]] + wpos[order]) >> HF_BIN_SHIFT) & (HF_SLOTS - 1)).astype(np.uint16)
    hv, hc = np.unique(ucount, return_counts=True)
    hist = {int(a): int(b) for a, b in zip(hv, hc)}

    # position directory: lower bounds of b << shift among each contig's positions, b = 0 .. (len >> shift) + 1
    shift = dir_shift_for(w)
    nb = (clen >> shift) + 2
    dir_off = np.zeros(C + 1, dtype=U64)
    dir_off[1:] = np.cumsum(nb)
    dc = np.repeat(np.arange(C, dtype=np.int64), nb)
    db = np.arange(int(dir_off[-1]), dtype=np.int64) - dir_off[:-1].astype(np.int64)[dc]
    key = (contig << 32) | wpos
    dir_ = (np.searchsorted(key, (dc << 32) | (db << shift), side="left") - cstart[:-1].astype(np.int64)[dc]).astype(U32)

    # duplicates: neighbours in a list that lie in one contig are a pair; DN on the earlier, DP on the later
    pw = pw0.copy()
    pair = np.nonzero((sh[:-1] == sh[1:]) & (contig[order][:-1] == contig[order][1:]))[0] if N > 1 else np.zeros(0, dtype=np.int64)
    oa, ob = order[pair], order[pair + 1]
    pw[oa] |= U32(PW_DN)
    pw[ob] |= U32(PW_DP)
    flagged = (pw & U32(PW_DP | PW_DN)) != 0
    nb64 = (N + 63) >> 6
    fl = np.zeros(nb64 * 64, dtype=np.uint8)
    fl[:N] = flagged
    dup_bits = np.packbits(fl.reshape(nb64, 64), axis=1, bitorder="little").view("<u8").reshape(nb64).astype(U64) if nb64 else np.zeros(0, dtype=U64)
    dup_rank = np.zeros(nb64 + 1, dtype=U64)
    dup_rank[1:] = np.cumsum(fl.reshape(nb64, 64).sum(axis=1)) if nb64 else 0
    n_flagged = int(flagged.sum())
    slot = np.cumsum(flagged) - 1
    dup_dist = np.zeros(n_flagged, dtype=U32)
    d = np.minimum(ob - oa, dup_sat).astype(U32)
    dup_dist[slot[oa]] |= d << U32(16)                              # "next" of the earlier entry
    dup_dist[slot[ob]] |= d                                         # "previous" of the later one
    prev_dist, next_dist = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    prev_dist[ob] = d
    next_dist[oa] = d

    # table: linear probing from the home slot, wrap at the end.  The occupied set and every hash's reachability do not depend on
    # the insertion order; which hash of a cluster sits where does.
    buckets = tab_buckets_for(U) if N else 64
    slots = buckets * 4
    home = tab_slot(uh, buckets)
    tab = np.zeros(2 * slots, dtype=U64)
    where = np.zeros(U, dtype=np.int64)
    taken = bytearray(slots)
    for u, s in enumerate(home.tolist()):
        while taken[s]:
            s = s + 1 if s + 1 < slots else 0
        taken[s] = 1
        where[u] = s
    tab[2 * where] = (ucount.astype(U64) << U64(32)) | uh.astype(U64)
    tab[2 * where + 1] = pstart[:-1].astype(U64)
    probe = (where - home) % slots if U else np.zeros(0, dtype=np.int64)

    return SimpleNamespace(k=k, w=w, C=C, N=N, U=U, P=P, contig_len=clen.astype(np.int32), cstart=cstart, hash=hash_, wpos=wpos.astype(np.int32), strand=strand,
                           contig=contig.astype(np.int32), pw=pw, pos=np.stack([hash_, pw], axis=1).astype(U32) if N else np.zeros((0, 2), dtype=U32),
                           uh=uh, ucount=ucount, ustart=ustart, pstart=pstart, sorted_hash=sh, occ=occ, occ16=occ16, hist=hist,
                           freq_threshold=freq_threshold(hist, U), dir_shift=shift, dir_off=dir_off, dir=dir_, n_dup=len(pair), n_flagged=n_flagged,
                           dup_bits=dup_bits, dup_rank=dup_rank, dup_dist=dup_dist, dup_sat=dup_sat, prev_dist=prev_dist, next_dist=next_dist,
                           pair_first=oa, pair_second=ob, tab_buckets=buckets, tab=tab, tab_home=home, tab_where=where,
                           longest_probe=int(probe.max()) if U else 0, wrapped=bool(np.any(where < home)))


def hist_arrays(model):
    ks = sorted(model.hist)
    return np.array(ks, dtype=np.int64), np.array([model.hist[c] for c in ks], dtype=np.int64)


def top16_max(model) -> int:
    """entries in the fullest 16-bit hash prefix: the smallest MM_INDEX_PART_MAX the partitioned sort accepts"""
    return int(np.bincount((model.hash >> U32(16)).astype(np.int64), minlength=1).max()) if model.N else 0


def partitions(model, part_max: int):
    """entry counts of the hash ranges the partitioned sort takes for this limit (None: the plain sort; raises where the build refuses)"""
    if model.N <= part_max:
        return None
    h16 = np.bincount((model.hash >> U32(16)).astype(np.int64), minlength=65536)
    if h16.max() > part_max:
        raise ValueError("one 16-bit hash prefix holds more entries than the limit")
    out, acc = [], 0
    for c in h16[np.nonzero(h16)[0]].tolist():
        if acc + c > part_max:
            out.append(acc); acc = 0
        acc += c
    out.append(acc)
    return [c for c in out if c]


# ---- the file ---------------------------------------------------------------------------------------
def stored_arrays(model) -> dict:
    """the ten arrays with the element counts index_build leaves them at (spare elements zero)"""
    N, P = model.N, model.P
    pad = lambda a, n: np.concatenate([a, np.zeros(n - len(a), dtype=a.dtype)])
    total_dir = int(model.dir_off[-1])
    return {"pos": model.pos.reshape(-1), "cstart": model.cstart,
            "occ": pad(model.occ, P + 2 if N else 1), "occ16": pad(model.occ16, P + 16 if N else 16), "tab": model.tab,
            "dir": pad(model.dir, max(total_dir, 1)), "dir_off": model.dir_off,
            "dup_bits": pad(model.dup_bits, max(len(model.dup_bits), 1)), "dup_rank": pad(model.dup_rank, len(model.dup_rank) if N else 2),
            "dup_dist": pad(model.dup_dist, max(model.n_flagged, 1))}


def write(path, model, freq_thr=None):
    hk, hn = hist_arrays(model)
    out = [MAGIC, struct.pack("<IiiiiiII", IDX_VERSION, model.k, model.w, model.dir_shift, model.dup_sat,
                              model.freq_threshold if freq_thr is None else freq_thr, model.tab_buckets, 0),
           struct.pack("<5q", model.C, model.N, model.U, model.n_dup, len(hk)),
           np.stack([hk, hn], axis=1).astype("<i8").tobytes(), model.contig_len.astype("<i4").tobytes(), model.cstart.astype("<u8").tobytes()]
    arrs = stored_arrays(model)
    for name, dt, _ in ARRAYS:
        raw = arrs[name].astype(dt).tobytes()
        count = len(raw) // np.dtype(dt).itemsize // (2 if name == "pos" else 1)
        out += [struct.pack("<QQ", count, array_sum(raw)), raw]
    out.append(struct.pack("<Q", IDX_TAIL))
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path


def parse(path) -> dict:
    data = bytes(path) if isinstance(path, (bytes, bytearray)) else open(path, "rb").read()   # (a file's bytes are taken as they are)
    assert data[:8] == MAGIC, "not an index file"
    version, k, w, dir_shift, dup_sat, thr, buckets, zero = struct.unpack_from("<IiiiiiII", data, 8)
    C, N, U, n_dup, n_hist = struct.unpack_from("<5q", data, 40)
    at = 80
    hist = np.frombuffer(data, dtype="<i8", count=2 * n_hist, offset=at).reshape(n_hist, 2); hist_at = at; at += 16 * n_hist
    contig_len = np.frombuffer(data, dtype="<i4", count=C, offset=at); at += 4 * C
    h_cstart = np.frombuffer(data, dtype="<u8", count=C + 1, offset=at); at += 8 * (C + 1)
    arrays = {}
    for name, dt, _ in ARRAYS:
        count, checksum = struct.unpack_from("<QQ", data, at)
        item = np.dtype(dt).itemsize * (2 if name == "pos" else 1)
        a = np.frombuffer(data, dtype=dt, count=count * (2 if name == "pos" else 1), offset=at + 16)
        arrays[name] = SimpleNamespace(count=count, checksum=checksum, offset=at + 16, nbytes=count * item, sum_at=at + 8,
                                       data=a.reshape(-1, 2) if name == "pos" else a)
        at += 16 + count * item
    (tail,) = struct.unpack_from("<Q", data, at)
    assert tail == IDX_TAIL and at + 8 == len(data), "index file without its closing word"
    return {"version": version, "k": k, "w": w, "dir_shift": dir_shift, "dup_sat": dup_sat, "freq_threshold": thr, "tab_buckets": buckets, "reserved": zero,
            "n_contigs": C, "N": N, "U": U, "n_dup": n_dup, "hist": hist, "hist_at": hist_at, "contig_len": contig_len, "h_cstart": h_cstart,
            "arrays": arrays, "bytes": data}


def edited(parsed, name, fn, fix_sum=True) -> bytes:
    """the file's bytes after fn changed a writable view of array `name` (pos: flat hash, pw words); fix_sum stores the new checksum"""
    buf, a = bytearray(parsed["bytes"]), parsed["arrays"][name]
    dt = np.dtype(ARRAY_DTYPE[name])
    fn(np.frombuffer(buf, dtype=dt, count=a.nbytes // dt.itemsize, offset=a.offset))
    if fix_sum:
        struct.pack_into("<Q", buf, a.sum_at, array_sum(bytes(buf[a.offset:a.offset + a.nbytes])))
    return bytes(buf)


def _first_diff(name, got, want, out):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        out.append((name, "length", got.shape, want.shape))
        return
    bad = np.nonzero(got != want)[0] if got.ndim == 1 else np.nonzero(np.any(got != want, axis=1))[0]
    if len(bad):
        i = int(bad[0])
        out.append((name, i, got[i].tolist(), want[i].tolist()))


def audit(parsed, model, freq_thr=None) -> list:
    """findings as (array, first offending index, value in the file, value of the model); empty when the file is right"""
    out, A = [], parsed["arrays"]
    want_head = {"version": IDX_VERSION, "k": model.k, "w": model.w, "dir_shift": model.dir_shift, "dup_sat": model.dup_sat,
                 "freq_threshold": model.freq_threshold if freq_thr is None else freq_thr, "tab_buckets": model.tab_buckets, "reserved": 0,
                 "n_contigs": model.C, "N": model.N, "U": model.U, "n_dup": model.n_dup}
    for f, v in want_head.items():
        if parsed[f] != v:
            out.append(("header", f, parsed[f], v))
    hk, hn = hist_arrays(model)
    _first_diff("hist", parsed["hist"], np.stack([hk, hn], axis=1), out)
    _first_diff("contig_len", parsed["contig_len"], model.contig_len, out)
    _first_diff("h_cstart", parsed["h_cstart"], model.cstart, out)
    N, P, U, total_dir = model.N, model.P, model.U, int(model.dir_off[-1])
    for name, want, n in (("pos", model.pos, N), ("cstart", model.cstart, model.C + 1), ("occ", model.occ, P), ("occ16", model.occ16, P),
                          ("dir", model.dir, total_dir), ("dir_off", model.dir_off, model.C + 1), ("dup_bits", model.dup_bits, len(model.dup_bits)),
                          ("dup_rank", model.dup_rank, len(model.dup_rank)), ("dup_dist", model.dup_dist, model.n_flagged)):
        if A[name].count < n:
            out.append((name, "count", A[name].count, n))
        else:
            _first_diff(name, A[name].data[:n], want[:n], out)
    # the table: which hash of a probe cluster sits in which slot is a race by design; occupancy and reachability are not
    slots = model.tab_buckets * 4
    if A["tab"].count != 2 * slots:
        out.append(("tab", "count", A["tab"].count, 2 * slots))
    else:
        w0, w1 = A["tab"].data[0::2], A["tab"].data[1::2]
        occupied, want_occ = w0 != 0, model.tab[0::2] != 0
        if int(occupied.sum()) != U:
            out.append(("tab", "occupied slots", int(occupied.sum()), U))
        _first_diff("tab", occupied, want_occ, out)
        foreign = np.nonzero(occupied & ~np.isin(w0 & U64(0xFFFFFFFF), model.uh.astype(U64)))[0]
        if len(foreign):
            out.append(("tab", int(foreign[0]), int(w0[foreign[0]]), "a hash the index lacks"))
        cur, found = model.tab_home.copy(), np.full(U, -1, dtype=np.int64)
        active, hq = np.ones(U, dtype=bool), model.uh.astype(U64)
        for _ in range(slots):
            if not active.any():
                break
            v = w0[cur]
            hit = active & ((v & U64(0xFFFFFFFF)) == hq) & (v != 0)
            found[hit] = cur[hit]
            active &= ~hit & (v != 0)
            cur = np.where(cur + 1 == slots, 0, cur + 1)
        lost = np.nonzero(found < 0)[0]
        if len(lost):
            out.append(("tab", int(model.tab_home[lost[0]]), "not reachable before an empty slot", int(model.uh[lost[0]])))
        ok = found >= 0
        _first_diff("tab", np.stack([w0[found[ok]] >> U64(32), w1[found[ok]]], axis=1),
                    np.stack([model.ucount[ok].astype(U64), model.pstart[:-1][ok].astype(U64)], axis=1), out)
    data = parsed["bytes"]
    for name, a in A.items():
        s = array_sum(data[a.offset:a.offset + a.nbytes])
        if s != a.checksum:
            out.append((name, "checksum", a.checksum, s))
    return out
