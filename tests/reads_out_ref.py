"""mapDirectly --extract-* / --deplete-taxa and mm_reads_encode, restated plainly (the definition: metamaps_amd/csrc/mm_reads_out_core.hpp and
host/reads_out.hpp): the bytes of one record, the three rules of the call, and which reads each of the four files takes, from the lines of a PREFIX."""
import gzip
import re

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def record(name: bytes, bases: bytes, quals, with_qual: bool) -> bytes:
    """bases: the bytes as given (upper-cased here, as the set does); quals: Phred values (0..93, or 0xFF for none) per base, or None for a read without"""
    bases = bases.upper()
    if not with_qual:
        return b">" + name + b"\n" + bases + b"\n"
    q = bytes(33 if v == 0xFF else v + 33 for v in quals) if quals is not None else b"!" * len(bases)
    assert len(q) == len(bases)
    return b"@" + name + b"\n" + bases + b"\n+\n" + q + b"\n"


def rule(read: int, n_reads: int, name: bytes):
    """the lowest rule the record breaks, or 0"""
    if read < 0 or read >= n_reads:
        return 1
    if len(name) < 1 or len(name) > 254:
        return 2
    if any(b < 0x21 or b > 0x7E for b in name):
        return 3
    return 0


def refusal(read, n_reads, names):
    """(record, rule) of the lowest record that breaks a rule, or None"""
    for i, (r, nm) in enumerate(zip(read, names)):
        k = rule(r, n_reads, nm)
        if k:
            return i, k
    return None


def text(reads, quals, selection, names, with_qual) -> bytes:
    """the inflated stream of one call: reads[i] the bases, quals[i] its Phred values or None"""
    assert refusal(selection, len(reads), names) is None
    return b"".join(record(nm, reads[r], quals[r], with_qual) for r, nm in zip(selection, names))


def inflate(data: bytes) -> bytes:
    return gzip.decompress(data) if data else b""


TAXON = re.compile(r"kraken:taxid\|(x?\d+)")


def taxon_of(contig: str) -> str:
    return TAXON.search(contig).group(1)


def primary_contigs(lines):
    """read ID -> the contig (field 6) of its primary line: the largest printed field 14, the first of equals"""
    best = {}
    for ln in lines:
        f = ln.split(" ")
        v = float(f[13])
        if f[0] not in best or v > best[f[0]][0]:
            best[f[0]] = (v, f[5])
    return {k: c for k, (_, c) in best.items()}


def selections(lines, ids, taxa):
    """the read indices (query order) of the four files, from the mapping lines of PREFIX, the IDs of all reads in query order and the taxon list (may be
    None: the two taxon files are not asked for)"""
    prim = primary_contigs(lines)
    out = {"mapped": [i for i, x in enumerate(ids) if x in prim], "unmapped": [i for i, x in enumerate(ids) if x not in prim]}
    if taxa is not None:
        hit = [i for i, x in enumerate(ids) if x in prim and taxon_of(prim[x]) in taxa]
        out["taxa"] = hit
        out["depleted"] = [i for i in range(len(ids)) if i not in set(hit)]
    return out
