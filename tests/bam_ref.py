"""The BAM records of mapDirectly --bam restated in plain Python (SAM/BAM specification v1.6; the device's text is metamaps_amd/csrc/mm_bam_core.hpp):
record() writes one record from the definition, decode() reads a whole file back with every field and tag, ref_from_md() rebuilds the reference
stretch an alignment covers from SEQ, CIGAR and MD alone.  Runs are BAM's words: len << 4 | op with I = 1, D = 2, = = 7, X = 8."""
import gzip
import math
import struct
import zlib

NT16 = "=ACMGRSVTWYHKDBN"
OP_I, OP_D, OP_N, OP_S, OP_EQ, OP_X = 1, 2, 3, 4, 7, 8
CIGAR_LETTER = "MIDNSHP=X"
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HD_LINE = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
PG_LINE = "@PG\tID:metamaps\tPN:metamaps\n"


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _ref_base(b):
    c = chr(b).upper()
    return c if "A" <= c <= "Z" else "N"


def md(contig_bytes, first, runs):
    """the MD string of the runs along contig_bytes from `first` on"""
    out, c, j = [], 0, first
    for w in runs:
        n, op = int(w) >> 4, int(w) & 15
        if op == OP_EQ:
            c += n
            j += n
        elif op == OP_X:
            for _ in range(n):
                out.append(f"{c}{_ref_base(contig_bytes[j])}")
                c = 0
                j += 1
        elif op == OP_D:
            out.append(f"{c}^" + "".join(_ref_base(b) for b in contig_bytes[j:j + n]))
            c = 0
            j += n
    out.append(str(c))
    return "".join(out)


def seq_codes(read, strand):
    """the 4-bit codes of SEQ: the read upper-cased, reversed and bit-reversed for strand -"""
    codes = [NT16.find(chr(b).upper()) if chr(b).upper() in NT16 else 15 for b in bytes(read)]
    if strand < 0:
        codes = [int(f"{c:04b}"[::-1], 2) for c in reversed(codes)]
    return codes


def record(name, read, strand, contig_index, contig_bytes, first, runs, d, flag, mapq):
    """one record, block_size included; name and read are bytes"""
    runs = [int(w) for w in runs]
    m = len(read)
    refspan = sum(w >> 4 for w in runs if (w & 15) in (OP_EQ, OP_X, OP_D))
    field = runs if len(runs) <= 65535 else [m << 4 | OP_S, refspan << 4 | OP_N]
    codes = seq_codes(read, strand) + [0]
    body = struct.pack("<iiBBHHHiiii", contig_index, first, len(name) + 1, mapq, reg2bin(first, first + refspan), len(field), flag, m, -1, -1, 0)
    body += bytes(name) + b"\0"
    body += struct.pack(f"<{len(field)}I", *field)
    body += bytes(codes[2 * i] << 4 | codes[2 * i + 1] for i in range((m + 1) // 2))
    body += b"\xff" * m
    body += b"NMi" + struct.pack("<i", d)
    body += b"MDZ" + md(contig_bytes, first, runs).encode() + b"\0"
    if len(runs) > 65535:
        body += b"CGBI" + struct.pack(f"<I{len(runs)}I", len(runs), *runs)
    return struct.pack("<i", len(body)) + body


def header(contigs):
    """the inflated header of PREFIX.bam for [(name, length)] (names as str)"""
    text = (HD_LINE + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in contigs) + PG_LINE).encode()
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs))
    for n, ln in contigs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return out


def members(data):
    """the BGZF members of a file, checked one by one: [(member bytes, inflated bytes)]"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert at + size <= len(data), "a member runs past the end"
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        raw = zlib.decompress(data[at + 18:at + size - 8], -15)
        assert len(raw) == isize and zlib.crc32(raw) == crc, at
        out.append((data[at:at + size], raw))
        at += size
    return out


def _tags(b):
    tags, at = {}, 0
    while at < len(b):
        key, typ = b[at:at + 2].decode(), chr(b[at + 2])
        at += 3
        if typ == "i":
            tags[key] = struct.unpack_from("<i", b, at)[0]
            at += 4
        elif typ == "Z":
            end = b.index(b"\0", at)
            tags[key] = b[at:end].decode()
            at = end + 1
        elif typ == "B":
            sub, n = chr(b[at]), struct.unpack_from("<I", b, at + 1)[0]
            assert sub == "I", sub
            tags[key] = list(struct.unpack_from(f"<{n}I", b, at + 5))
            at += 5 + 4 * n
        else:
            raise AssertionError(f"tag type {typ}")
    return tags


def decode_records(raw):
    """the records of an inflated stretch that holds whole records: a dict of every field each"""
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<i", raw, at)[0]
        refid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, at + 4)
        p = at + 36
        name = raw[p:p + l_name - 1]
        assert raw[p + l_name - 1] == 0
        p += l_name
        cig = list(struct.unpack_from(f"<{n_cig}I", raw, p))
        p += 4 * n_cig
        packed = raw[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(NT16[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        assert l_seq % 2 == 0 or packed[-1] & 15 == 0
        qual = raw[p:p + l_seq]
        p += l_seq
        tag_bytes = raw[p:at + 4 + size]
        tags = _tags(tag_bytes)
        out.append(dict(refID=refid, pos=pos, mapq=mapq, bin=bin_, flag=flag, l_seq=l_seq, next_refID=nref, next_pos=npos, tlen=tlen, name=name, cigar_field=cig,
                        cigar=tags.get("CG", cig), seq=seq, qual=qual, tags=tags, tag_order=[tag_bytes[i:i + 2].decode() for i in _tag_starts(tag_bytes)]))
        at += 4 + size
    assert at == len(raw)
    return out


def _tag_starts(b):
    at, out = 0, []
    while at < len(b):
        out.append(at)
        typ = chr(b[at + 2])
        at += 3
        at = at + 4 if typ == "i" else b.index(b"\0", at) + 1 if typ == "Z" else at + 5 + 4 * struct.unpack_from("<I", b, at + 1)[0]
    return out


def decode(stream):
    """a whole .bam file (bytes) -> (header_text, [(contig name, length)], records); the file ends with the EOF block"""
    assert stream.endswith(EOF_BLOCK)
    raw = b"".join(r for _, r in members(stream))
    assert raw == gzip.decompress(stream)
    assert raw[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].decode()
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, at)[0]
        refs.append((raw[at + 4:at + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, at + 4 + l_name)[0]))
        at += 8 + l_name
    return text, refs, decode_records(raw[at:])


def cigar_string(runs):
    return "".join(f"{int(w) >> 4}{CIGAR_LETTER[int(w) & 15]}" for w in runs)


def ref_from_md(seq, cigar, md_text):
    """the reference stretch under the alignment: = bases from SEQ, X and D bases from MD; checks that MD and the CIGAR agree run for run"""
    import re
    assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", md_text), md_text
    items = re.findall(r"[0-9]+|\^[A-Z]+|[A-Z]", md_text)
    k, left, out, i = 0, int(items[0]), [], 0                       # left: matched bases the current number still covers
    for w in cigar:
        n, op = int(w) >> 4, int(w) & 15
        if op == OP_I:
            i += n
        elif op == OP_EQ:
            assert left >= n, "MD's match count is shorter than the = run"
            out.append(seq[i:i + n])
            left -= n
            i += n
        elif op == OP_X:
            for _ in range(n):
                assert left == 0 and len(items[k + 1]) == 1
                out.append(items[k + 1])
                left = int(items[k + 2])
                k += 2
                i += 1
        elif op == OP_D:
            assert left == 0 and items[k + 1] == "^" + items[k + 1][1:] and len(items[k + 1]) == n + 1
            out.append(items[k + 1][1:])
            left = int(items[k + 2])
            k += 2
        else:
            raise AssertionError(f"op {op}")
    assert left == 0 and k == len(items) - 1 and i == len(seq)
    return "".join(out)


def mapq_from_text(field14):
    q = float(field14)
    if q <= 0:
        return 0
    if 1 - q <= 1e-6:
        return 60
    return min(60, int(math.floor(-10 * math.log10(1 - q) + 0.5)))
