"""The error profile of mapDirectly --error-profile, restated plainly: one column of the alignment at a time, dicts and lists of Python integers.  It shares
no code with metamaps_amd/csrc/mm_errprof_core.hpp; tests/test_errprof_core.py holds the header's host form to it, tests/test_gpu_errprof.py the device,
tests/test_errprof_out.py the four writers and tests/test_gpu_cli_errprof.py the files of the command line.

A job is pileup_ref.py's dict (read: the bytes its set holds, strand, c, first, runs, d, use) with an optional qual: the stored qualities of its read, one
integer 0..93 per base, or None."""
import math

LETTERS = "ACGTN"
COUNTERS = 566
NO_KEY = (1 << 64) - 1
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def letter(byte):
    ch = chr(byte).upper()
    return ch if ch in "ACGT" else "N"


def contributes(j):
    return j.get("use", 1) != 0 and j["d"] >= 0


def empty_tables():
    return dict(sub=[[0] * 5 for _ in range(5)], indel=[[[0] * 64 for _ in range(2)] for _ in range(2)], qual=[[0] * 95 for _ in range(3)])


def job_profile(j, contig, t):
    """adds the job's columns to the tables t; returns its six columns"""
    m = len(j["read"])
    stored = [letter(b) for b in j["read"]]                         # what the sequencer wrote
    squal = j.get("qual")
    squal = [94] * m if squal is None else list(squal)
    if j["strand"] < 0:                                             # the oriented read: base i is stored base m - 1 - i, complemented
        seen, q, ql = stored[::-1], [_COMP[ch] for ch in reversed(stored)], squal[::-1]
    else:
        seen, q, ql = stored, stored, squal
    ref = [letter(b) for b in contig]
    r, i = j["first"], 0
    eq = x = ins_runs = ins_bases = del_runs = del_bases = 0
    for w in j["runs"]:
        n, op = int(w) >> 4, int(w) & 15
        if op in (7, 8):
            for _ in range(n):
                truth = _COMP[ref[r]] if j["strand"] < 0 else ref[r]
                t["sub"][LETTERS.index(truth)][LETTERS.index(seen[i])] += 1
                t["qual"][0 if op == 7 else 1][ql[i]] += 1
                r += 1; i += 1
            if op == 7:
                eq += n
            else:
                x += n
        elif op == 1:
            bases = q[i:i + n]
            for k in range(n):
                t["qual"][2][ql[i + k]] += 1
            b = bases[0]
            hp = b in "ACGT" and all(ch == b for ch in bases) and ((r >= 1 and ref[r - 1] == b) or (r < len(ref) and ref[r] == b))
            t["indel"][0][1 if hp else 0][min(n, 64) - 1] += 1
            ins_runs += 1; ins_bases += n; i += n
        elif op == 2:
            bases = ref[r:r + n]
            b = bases[0]
            hp = b in "ACGT" and all(ch == b for ch in bases) and ((r >= 1 and ref[r - 1] == b) or (r + n < len(ref) and ref[r + n] == b))
            t["indel"][1][1 if hp else 0][min(n, 64) - 1] += 1
            del_runs += 1; del_bases += n; r += n
        else:
            raise ValueError(w)
    assert i == m
    return [eq, x, ins_runs, ins_bases, del_runs, del_bases]


def ident_key(c, cols):
    den = cols[0] + cols[1] + cols[3] + cols[5]
    return c << 32 | (1_000_000 * cols[0] // den if den else 0)


def profile(jobs, contigs):
    """(counters [566], cols [[6] per job], keys [per job]) of the jobs in order"""
    t = empty_tables()
    cols, keys = [], []
    for j in jobs:
        if contributes(j):
            c = job_profile(j, contigs[j["c"]], t)
            cols.append(c); keys.append(ident_key(j["c"], c))
        else:
            cols.append([0] * 6); keys.append(NO_KEY)
    return flat(t), cols, keys


def flat(t):
    out = [v for row in t["sub"] for v in row] + [v for kind in t["indel"] for hp in kind for v in hp] + [v for cls in t["qual"] for v in cls]
    assert len(out) == COUNTERS
    return out


def unflat(counters):
    c = [int(v) for v in counters]
    assert len(c) == COUNTERS
    return dict(sub=[c[5 * a:5 * a + 5] for a in range(5)], indel=[[c[25 + (k * 2 + h) * 64:25 + (k * 2 + h) * 64 + 64] for h in range(2)] for k in range(2)],
                qual=[c[281 + 95 * s:281 + 95 * s + 95] for s in range(3)])


def row_of(entries):
    """[alignments, six sums, min, q1, median, q3, max] of (ppm, cols) entries; zeros of none"""
    n = len(entries)
    if n == 0:
        return [0] * 12
    v = sorted(p for p, _ in entries)
    return [n] + [sum(c[k] for _, c in entries) for k in range(6)] + [v[0], v[(n - 1) // 4], v[(n - 1) // 2], v[3 * (n - 1) // 4], v[n - 1]]


def finish(keys, cols):
    """(contigs listed ascending, their rows, the row of all alignments) of the entries whose key is not NO_KEY"""
    by = {}
    for k, c in zip(keys, cols):
        if int(k) != NO_KEY:
            by.setdefault(int(k) >> 32, []).append((int(k) & 0xFFFFFFFF, [int(v) for v in c]))
    listed = sorted(by)
    return listed, [row_of(by[c]) for c in listed], row_of([e for c in listed for e in by[c]])


# ---- the four files
SUB_HEADER = "#truth\tA\tC\tG\tT\tN\n"
INDEL_HEADER = "#kind\tlength\thomopolymer\tother\n"
QUAL_HEADER = "#quality\tmatches\tmismatches\tinserted\terrorRate\tempiricalQ\n"
CONTIGS_HEADER = ("#contigID\tlength\talignments\treadBases\trefBases\tmatches\tmismatches\tinsertions\tinsertedBases\tdeletions\tdeletedBases\tidentity\tgapCompressedIdentity"
                  "\tminIdentity\tq1Identity\tmedianIdentity\tq3Identity\tmaxIdentity\n")


def substitutions_text(t):
    if not any(any(row) for row in t["sub"]):
        return SUB_HEADER
    return SUB_HEADER + "".join(LETTERS[a] + "".join(f"\t{v}" for v in t["sub"][a]) + "\n" for a in range(5))


def indels_text(t):
    out = [INDEL_HEADER]
    for kind, name in ((0, "I"), (1, "D")):
        for n in range(64):
            hp, other = t["indel"][kind][1][n], t["indel"][kind][0][n]
            if hp or other:
                out.append(f"{name}\t{'64+' if n == 63 else n + 1}\t{hp}\t{other}\n")
    return "".join(out)


def qualities_text(t):
    out = [QUAL_HEADER]
    for row in range(95):
        eq, x, ins = (t["qual"][s][row] for s in range(3))
        if eq + x + ins == 0:
            continue
        rate = (x + ins) / (eq + x + ins)
        out.append(f"{'none' if row == 94 else row}\t{eq}\t{x}\t{ins}\t{rate:.6f}\t{'inf' if x + ins == 0 else format(-10 * math.log10(rate) + 0.0, '.2f')}\n")
    return "".join(out)


def contig_line(name, length, row):
    n, eq, x, ir, ib, dr, db = row[:7]
    ident = eq / (eq + x + ib + db) if eq + x + ib + db else 0.0
    gap = eq / (eq + x + ir + dr) if eq + x + ir + dr else 0.0
    nums = [ident, gap] + [p / 1e6 for p in row[7:]]
    return f"{name}\t{length}\t{n}\t{eq + x + ib}\t{eq + x + db}\t{eq}\t{x}\t{ir}\t{ib}\t{dr}\t{db}" + "".join(f"\t{v:.6f}" for v in nums) + "\n"


def contigs_text(listed, rows, total, cname, clen):
    if not listed:
        return CONTIGS_HEADER
    return CONTIGS_HEADER + "".join(contig_line(cname[c], clen[c], r) for c, r in zip(listed, rows)) + contig_line("*", sum(clen[c] for c in listed), total)
