"""The consensus of mapDirectly --consensus, restated plainly: strings, lists and dicts, one contig after the other and one candidate after the other.  It
shares no code with metamaps_amd/csrc/mm_cons_core.hpp or host/consensus_out.hpp; tests/test_cons_core.py holds the header's host form to it,
tests/test_gpu_consensus.py the device, and tests/test_gpu_cli_consensus.py the two files of the command line.

A table is vcf_ref.py's {(w0, w1): count}; intervals are (contig, first, last); contigs is the list of the reference's byte strings."""
import math

DEL, INS = 5, 6
EXPLICIT_MAX = 24
STATS = ("alignments", "called", "written", "consensusLength", "snvs", "deletions", "deletedBases", "insertions", "insertedBases", "dropped")
TSV_HEADER = "contigID\tlength\t" + "\t".join(STATS) + "\n"


def depths(intervals, c, n):
    d = [0] * n
    for cc, a, b in intervals:
        if cc == c:
            for p in range(a, b + 1):
                d[p] += 1
    return d


def contig(t, intervals, c, seq, min_depth, min_frac, min_called):
    """one contig with an interval: (stats dict, consensus string or None where it is not written, {reference position: column of its base})"""
    n = len(seq)
    d = depths(intervals, c, n)
    rows = [(k[0] >> 3 & 0xFFFFFFFF, k[0] & 7, k[1], t[k]) for k in sorted(t) if k[0] >> 35 == c]
    cand = [r for r in rows if d[r[0]] >= min_depth and float(r[3]) >= min_frac * float(d[r[0]])]
    removed, snv, ins = set(), {}, {}
    s = dict.fromkeys(STATS, 0)
    s["alignments"] = sum(1 for cc, _, _ in intervals if cc == c)
    s["called"] = sum(1 for x in d if x >= min_depth)
    end = -1                                                        # the largest footprint end of the candidate deletions so far, applied or not
    for pos, code, w1, _ in cand:
        if code == DEL:
            if pos + 1 > end:
                removed.update(range(pos + 1, pos + w1 + 1))
                s["deletions"] += 1
                s["deletedBases"] += w1
            end = max(end, pos + w1)
    seen_snv, seen_ins = set(), set()
    for pos, code, w1, _ in cand:
        if code < 4:
            if pos not in removed and pos not in seen_snv:
                snv[pos] = "ACGT"[code]
                s["snvs"] += 1
            seen_snv.add(pos)
        elif code == INS:
            if pos not in removed and pos not in seen_ins:
                m = w1 >> 48
                ins[pos] = "".join("ACGT"[w1 >> 2 * k & 3] for k in range(m)) if m <= EXPLICIT_MAX else "N" * m
                s["insertions"] += 1
                s["insertedBases"] += m
            seen_ins.add(pos)
    s["dropped"] = len(cand) - s["snvs"] - s["deletions"] - s["insertions"]
    letters = bytes(seq).decode("latin-1").upper()
    out, col = [], {}
    for p in range(n):
        if p in removed:
            continue
        if p in snv:
            out.append(snv[p])
        elif d[p] < min_depth:
            out.append("N")
        else:
            out.append(letters[p] if letters[p] in "ACGT" else "N")
        if p in ins:
            out.append(ins[p])
    at = 0
    for p in range(n):                                              # the column of every position that is not removed
        if p in removed:
            continue
        col[p] = at
        at += 1 + len(ins.get(p, ""))
    text = "".join(out)
    assert at == len(text) == n - s["deletedBases"] + s["insertedBases"]
    written = s["called"] >= max(1, math.ceil(min_called * n))
    s["written"] = int(written)
    s["consensusLength"] = len(text) if written else 0
    return s, (text if written else None), col


def wrapped(text, width):
    return "".join(text[i:i + width] + "\n" for i in range(0, len(text), width))


def consensus(t, intervals, contigs, min_depth, min_frac, min_called):
    """{contig: (stats, consensus or None, columns)} for every contig with an interval"""
    return {c: contig(t, intervals, c, contigs[c], min_depth, min_frac, min_called) for c in sorted({cc for cc, _, _ in intervals})}


def fasta_text(result, cname, width=60):
    """PREFIX.consensus.fa of consensus()'s result"""
    return "".join(f">{cname[c]}\n" + wrapped(text, width) for c, (_, text, _) in sorted(result.items()) if text is not None).encode("latin-1")


def tsv_text(result, cname, clen):
    """PREFIX.consensus.tsv"""
    return (TSV_HEADER + "".join(f"{cname[c]}\t{clen[c]}\t" + "\t".join(str(s[k]) for k in STATS) + "\n" for c, (s, _, _) in sorted(result.items()))).encode("latin-1")
