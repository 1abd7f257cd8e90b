"""The BAI index of a coordinate-sorted BAM restated in plain Python (SAM specification section 5.2, with the canonical choices of
include/metamaps_hip.h, mm_bam_sorter_*): build() makes the index's bytes from a BAM file's bytes, parse() reads an index back, query() follows the
specification's reg2bins + linear-index procedure.  The device's text is metamaps_amd/csrc/mm_bam_sort_core.hpp."""
import struct

import bam_ref

PSEUDO_BIN = 37450


def header_end(raw):
    """(reference lengths, offset of the first record) of an inflated BAM"""
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    lens = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, at)[0]
        lens.append(struct.unpack_from("<i", raw, at + 4 + l_name)[0])
        at += 8 + l_name
    return lens, at


def bam_coords(raw):
    """[(ref, beg, end, bytes)] of the records of an inflated stretch of real records: end = pos + max(1, reference span)"""
    out, at = [], 0
    for r in bam_ref.decode_records(raw):
        span = sum(w >> 4 for w in r["cigar"] if (w & 15) in (0, 2, 3, 7, 8))
        size = 4 + struct.unpack_from("<i", raw, at)[0]
        out.append((r["refID"], r["pos"], r["pos"] + max(1, span), size))
        at += size
    return out


def placed(data, coords=bam_coords):
    """(reference lengths, [(ref, beg, end, vs, ve)] in file order) of a BAM file's bytes.  A virtual offset is (file offset of the member that holds the
    byte) << 16 | (offset in that member's inflated bytes); the byte after the stream's last lies in the end-of-file block."""
    ms = bam_ref.members(data)
    assert ms and ms[-1][0] == bam_ref.EOF_BLOCK
    file_at, raw_at, f, r = [], [], 0, 0
    for m, raw in ms:
        file_at.append(f); raw_at.append(r)
        f += len(m); r += len(raw)

    def voff(x):
        for k in range(len(ms)):
            if raw_at[k] <= x < raw_at[k] + len(ms[k][1]):
                return file_at[k] << 16 | (x - raw_at[k])
        assert x == r
        return file_at[-1] << 16
    raw = b"".join(x for _, x in ms)
    lens, at = header_end(raw)
    recs = []
    for ref, beg, end, size in coords(raw[at:]):
        recs.append((ref, beg, end, voff(at), voff(at + size)))
        at += size
    assert at == len(raw)
    return lens, recs


def build(data, coords=bam_coords):
    lens, recs = placed(data, coords)
    out = b"BAI\1" + struct.pack("<i", len(lens))
    for r in range(len(lens)):
        mine = [(i, x) for i, x in enumerate(recs) if x[0] == r]
        if not mine:
            out += struct.pack("<ii", 0, 0)
            continue
        bins, last = {}, {}
        for i, (_, beg, end, vs, ve) in mine:
            b = bam_ref.reg2bin(beg, end)
            if b in bins and last[b] == i - 1:
                bins[b][-1] = (bins[b][-1][0], ve)
            else:
                bins.setdefault(b, []).append((vs, ve))
            last[b] = i
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", vs, ve) for vs, ve in bins[b])
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, mine[0][1][3], mine[-1][1][4], len(mine), 0)
        n_intv = 1 + ((max(x[2] for _, x in mine) - 1) >> 14)
        ioff = [None] * n_intv
        for w in range(n_intv):
            for _, (_, beg, end, vs, _) in mine:
                if beg < (w + 1) << 14 and end > w << 14:
                    ioff[w] = vs
                    break
        for w in range(n_intv - 2, -1, -1):
            if ioff[w] is None:
                ioff[w] = ioff[w + 1]
        assert None not in ioff
        out += struct.pack("<i", n_intv) + struct.pack(f"<{n_intv}Q", *ioff)
    return out + struct.pack("<Q", 0)


def parse(bai):
    """[dict(bins={bin: [(vs, ve)]}, pseudo=[(..), (..)] or None, ioff=[...])] per reference; checks the framing"""
    assert bai[:4] == b"BAI\1"
    n_ref, at, out = struct.unpack_from("<i", bai, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, at)[0]
        at += 4
        bins, pseudo, order = {}, None, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == PSEUDO_BIN:
                pseudo = chunks
            else:
                assert pseudo is None and b not in bins
                bins[b] = chunks
                order.append(b)
        assert order == sorted(order)
        n_intv = struct.unpack_from("<i", bai, at)[0]
        ioff = list(struct.unpack_from(f"<{n_intv}Q", bai, at + 4))
        at += 4 + 8 * n_intv
        out.append(dict(bins=bins, pseudo=pseudo, ioff=ioff))
    assert struct.unpack_from("<Q", bai, at)[0] == 0 and at + 8 == len(bai)
    return out


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query(bai, ref, beg, end):
    """the chunks [(vs, ve)] a reader visits for [beg, end) of reference `ref`: those of the bins of reg2bins that end behind the linear index's offset
    for beg's window, ascending; `bai` is parse()'s list"""
    idx = bai[ref]
    w = beg >> 14
    if w >= len(idx["ioff"]):
        return []                                                   # no record of the reference ends behind beg
    low = idx["ioff"][w]
    return sorted((max(vs, low), ve) for b in reg2bins(beg, end) for vs, ve in idx["bins"].get(b, []) if ve > low)
