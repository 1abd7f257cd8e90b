"""The pileup of mapDirectly --pileup, restated plainly: a dict of counts, and depth by looping over the intervals.  It shares no code with
metamaps_amd/csrc/mm_pileup_core.hpp; tests/test_pileup_core.py holds the header's host form to it, tests/test_gpu_pileup.py the device, and
tests/test_gpu_cli_pileup.py the two files of the command line.

A job is a dict with read (the bytes its set holds), strand, c (the contig's index), first, runs (len << 4 | op words) and d; use (default 1) says
whether it is its read's primary record."""

ALT = "ACGTN-+"
DEL, INS = 5, 6
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def oriented(read, strand):
    """the read as it is aligned, one letter of ACGTN per base"""
    s = [ch if ch in "ACGT" else "N" for ch in bytes(read).decode("latin-1").upper()]
    if strand < 0:
        s = [_COMP.get(ch, "N") for ch in reversed(s)]
    return s


def key(contig, pos, code):
    return contig << 35 | pos << 3 | code


def unkey(k):
    return int(k) >> 35, (int(k) >> 3) & 0xFFFFFFFF, int(k) & 7


def contributes(j):
    return j.get("use", 1) != 0 and j["d"] >= 0


def events(j):
    """the events of one contributing alignment as (contig, pos, code), in the order of the walk"""
    q = oriented(j["read"], j["strand"])
    r, i, out = j["first"], 0, []
    for w in j["runs"]:
        n, op = int(w) >> 4, int(w) & 15
        if op == 7:
            r += n; i += n
        elif op == 8:
            for t in range(n):
                out.append((j["c"], r + t, "ACGTN".index(q[i + t])))
            r += n; i += n
        elif op == 2:
            for t in range(n):
                out.append((j["c"], r + t, DEL))
            r += n
        elif op == 1:
            out.append((j["c"], r - 1 if r > j["first"] else j["first"], INS))
            i += n
        else:
            raise ValueError(w)
    assert i == len(q)
    return out


def interval(j):
    """(contig, first, last) of a contributing alignment"""
    span = sum(int(w) >> 4 for w in j["runs"] if int(w) & 15 != 1)
    return j["c"], j["first"], j["first"] + span - 1


def table(jobs):
    """{key: count} over the contributing jobs"""
    t = {}
    for j in jobs:
        if contributes(j):
            for e in events(j):
                t[key(*e)] = t.get(key(*e), 0) + 1
    return t


def merged(pairs):
    t = {}
    for k, c in pairs:
        t[int(k)] = t.get(int(k), 0) + int(c)
    return t


def depth(intervals, contig, pos):
    return sum(1 for c, a, b in intervals if c == contig and a <= pos <= b)


def finish(t, intervals, clen, min_count, min_frac):
    """(sites, contigs): sites [(key, count, depth)] in key order, those with count >= min_count and count >= min_frac * depth; contigs
    [(alignments, covered, sum_depth)] for every contig"""
    sites = []
    for k in sorted(t):
        c, pos, _ = unkey(k)
        d = depth(intervals, c, pos)
        if t[k] >= min_count and float(t[k]) >= min_frac * float(d):
            sites.append((k, t[k], d))
    contigs = []
    for c, n in enumerate(clen):
        hit = bytearray(n)
        mine = [(a, b) for cc, a, b in intervals if cc == c]
        for a, b in mine:
            hit[a:b + 1] = b"\1" * (b + 1 - a)
        contigs.append((len(mine), sum(hit), sum(b - a + 1 for a, b in mine)))
    return sites, contigs


def pileup_text(sites, cname, contig_bytes):
    """PREFIX.pileup: contigID pos ref alt count depth"""
    out = []
    for k, n, d in sites:
        c, pos, code = unkey(k)
        out.append(f"{cname[c]}\t{pos}\t{chr(contig_bytes[c][pos])}\t{ALT[code]}\t{n}\t{d}\n")
    return "".join(out).encode("latin-1")


def contigs_text(contigs, cname, clen):
    """PREFIX.pileup.contigs: contigID length alignments covered sumDepth, for the contigs with an alignment"""
    return "".join(f"{cname[c]}\t{clen[c]}\t{a}\t{cov}\t{s}\n" for c, (a, cov, s) in enumerate(contigs) if a).encode("latin-1")
