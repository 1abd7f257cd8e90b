"""Record sets for the tests of the BAM sorter (mm_bam_sorter_*; metamaps_amd/csrc/mm_bam_sort_core.hpp).  The sorter never looks inside a record beyond
its size, so a record here is block_size, then ref, pos and end as three int32 (where a real record has refID, pos and the bin word), then random bytes.
A case is dict(ref_len=[...], runs=[[record bytes, ...], ...]) with every run ascending by (ref, pos)."""
import struct

import numpy as np

import bam_ref
import bam_writer

MEMBER = 65280
LONG = (1 << 29) - 1                                                # the longest contig a BAI holds


def header(ref_len):
    """the inflated header of a coordinate-sorted file over contigs c0, c1, ... of these lengths: bam_ref.header's with the sorted first line"""
    names = ["c%d" % r for r in range(len(ref_len))]
    text = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in zip(names, ref_len)) + bam_ref.PG_LINE).encode()
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(ref_len)) + b"".join(
        struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln) for n, ln in zip(names, ref_len))


def record(rng, ref, pos, end, size):
    assert size >= 36 and 0 <= pos < end
    return struct.pack("<iiii", size - 4, ref, pos, end) + rng.bytes(size - 16)


def coords(raw):
    """[(ref, beg, end, bytes)] of an inflated stretch of these records (bai_ref.placed's `coords`)"""
    out, at = [], 0
    while at < len(raw):
        size, ref, pos, end = struct.unpack_from("<iiii", raw, at)
        out.append((ref, pos, end, size + 4))
        at += size + 4
    assert at == len(raw)
    return out


def run_arrays(records, block=50001):
    """(members of the run made by zlib in blocks of `block` bytes, raw_off, ref, pos, end)"""
    raw = b"".join(records)
    bgzf = b"".join(bam_writer.bgzf_block(raw[a:a + block], 1) for a in range(0, len(raw), block))
    raw_off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.int64)
    cs = coords(raw)
    return bgzf, raw_off, [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]


def sorted_stream(case):
    """the records in the defined order: ascending (ref, pos), then run, then index in the run"""
    keyed = [(coords(rec)[0][:2], r, i, rec) for r, run in enumerate(case["runs"]) for i, rec in enumerate(run)]
    return [rec for _, _, _, rec in sorted(keyed, key=lambda k: (k[0], k[1], k[2]))]


def deal(records, n_runs, rng):
    """records (ascending) dealt onto n_runs runs at random: every run stays ascending"""
    runs = [[] for _ in range(n_runs)]
    for rec in records:
        runs[int(rng.integers(0, n_runs))].append(rec)
    return runs


def edges(seed=91):
    """three runs over five references, two of them without records between ones that have them: records that end on a member's edge and one byte to
    either side, sizes from 36 to one above three members, positions at the window and bin edges up to the end of the longest contig"""
    rng = np.random.default_rng(seed)
    recs, pos = [], 0
    for size in (36, 37, 38, 39, MEMBER - 150, MEMBER - 1, 37, MEMBER - 36 + 1, MEMBER, MEMBER + 1, 3 * MEMBER + 1, 36, 41):   # ends at 1 M, 2 M - 1, 3 M + 1, ...
        recs.append(record(rng, 0, pos, pos + 1 + int(rng.integers(0, 3000)), size))
        pos += 1 + int(rng.integers(0, 2))                          # (ascending: the order of these is the order here)
    for p in (0, (1 << 14) - 1, 1 << 14, 1 << 17, 1 << 26, LONG - 1):
        for span in (1, 20000, 1 << 18):
            recs.append(record(rng, 2, p, min(LONG, p + span), 36 + int(rng.integers(0, 200))))
    at = 0
    for _ in range(220):                                            # dense small records: every pairing of byte residues, many records per wavefront
        at += int(rng.integers(0, 9000))
        recs.append(record(rng, 4, at, at + 1 + int(rng.integers(0, 40000)), 36 + int(rng.integers(0, 120))))
    return dict(ref_len=[70000, 5, LONG, 0, 3_000_000], runs=deal(recs, 3, rng))


def ties(seed=92):
    """seventeen runs, some empty, every record with the same key: the order is by run, then by index"""
    rng = np.random.default_rng(seed)
    runs = [[record(rng, 1, 5, 9, 36 + int(rng.integers(0, 5000))) for _ in range(0 if r % 5 == 2 else int(rng.integers(1, 6)))] for r in range(17)]
    return dict(ref_len=[10, 10], runs=runs)


def one_run(seed=93):
    rng = np.random.default_rng(seed)
    recs = [record(rng, k // 20, 100 * (k % 20), 100 * (k % 20) + 250, 36 + int(rng.integers(0, 9000))) for k in range(60)]
    return dict(ref_len=[5000, 5000, 5000], runs=[recs])


def nothing():
    return dict(ref_len=[100, 200], runs=[[], [], []])


def regions(case, n=300, seed=94):
    """(ref, beg, end) to ask an index for: seeded ones over the references, and the edges of the windows and of the bins around the records"""
    rng = np.random.default_rng(seed)
    out = []
    lens = [(r, ln) for r, ln in enumerate(case["ref_len"]) if ln > 0]
    for _ in range(n):
        r, ln = lens[int(rng.integers(0, len(lens)))]
        beg = int(rng.integers(0, ln)) if rng.random() < 0.5 else int(rng.integers(0, min(ln, 200000)))
        out.append((r, beg, min(ln, beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 20)))))))
    for r, ln in lens:
        for shift in (14, 17, 20, 23, 26):
            for e in {1 << shift, 2 << shift, ((ln - 1) >> shift) << shift}:
                for a, b in ((e - 1, e), (e, e + 1), (e - 1, e + 1)):
                    if 0 <= a < b <= ln:
                        out.append((r, a, b))
        out += [(r, 0, 1), (r, ln - 1, ln), (r, 0, ln)]
    return out
