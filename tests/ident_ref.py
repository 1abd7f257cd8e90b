"""The identity filter of DESIGN.md section 4 ("Identity filter") restated in Python, for the tests of mm_ident_core.hpp, mm_ident_filter and
`classify --min-identity`.  Two restatements:
  filter_arrays   arrays in, arrays out — what mm_ident_filter computes, naively: per-taxon Python lists, sorted(x)[len(x) // 2]
  recompute       text in, text out — every file `classify --min-identity T` writes that needs no EM, from PREFIX, PREFIX.EM, PREFIX.EM.WIMP,
                  PREFIX.EM.reads2Taxon and the DB's taxonomy; with refit=True also what of the refit follows without an EM: the kept lines
Nothing here shares code with the product."""
import os
import re

import numpy as np

TAXID = re.compile(r"kraken:taxid\|(x?\d+)")


def filter_arrays(read_off, taxon, ident, best, n_taxa, thr):
    read_off = [int(x) for x in read_off]
    taxon = [int(x) for x in taxon]
    ident = [float(x) + 0.0 for x in ident]                         # (-0.0 is 0)
    n_reads = len(read_off) - 1
    read_max, per = [], [[] for _ in range(n_taxa)]
    for r in range(n_reads):
        a, b = read_off[r], read_off[r + 1]
        if b > a:
            read_max.append(max(ident[a:b]))
            per[taxon[int(best[r])]].append(ident[int(best[r])])
    sorted_max = sorted(read_max)
    taxon_reads = [len(x) for x in per]
    taxon_median = [sorted(x)[len(x) // 2] if x else float("nan") for x in per]
    removed = [len(x) > 0 and m < thr for x, m in zip(per, taxon_median)]
    read_removed, read_src, entry_src, off_out = [], [], [], [0]
    for r in range(n_reads):
        a, b = read_off[r], read_off[r + 1]
        read_removed.append(b > a and removed[taxon[int(best[r])]])
        keep = [i for i in range(a, b) if not removed[taxon[i]]]
        if keep:
            read_src.append(r)
            entry_src += keep
            off_out.append(len(entry_src))
    i8 = lambda x: np.array(x, dtype=np.int64)
    return dict(sorted_max=np.array(sorted_max, dtype=np.float64), n_le=sum(1 for x in read_max if x <= thr), taxon_reads=i8(taxon_reads),
                taxon_median=np.array(taxon_median, dtype=np.float64), taxon_removed=np.array(removed, dtype=bool),
                read_removed=np.array(read_removed, dtype=bool), read_src=i8(read_src), entry_src=i8(entry_src), read_off_out=i8(off_out))


def same(got, want, filtered=True):
    """every result of mm_ident_filter (or of the host build) equals the restatement's, exactly"""
    keys = ["sorted_max", "taxon_reads", "taxon_removed", "read_removed"] + (["read_src", "entry_src", "read_off_out"] if filtered else [])
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    assert np.array_equal(np.asarray(got["taxon_median"]), want["taxon_median"], equal_nan=True)
    assert int(got["n_le"]) == want["n_le"]


# ---- text level

def read_groups(path):
    """the mapping lines of a file as lists of fields, read by read"""
    reads, cur = [], None
    for ln in open(path):
        ln = ln.rstrip("\n")
        if not ln:
            continue
        f = ln.split(" ")
        if f[0] != cur:
            cur = f[0]
            reads.append([])
        reads[-1].append(f)
    return reads


def best_lines(em_reads, r2t):
    """the index of every read's best line in PREFIX.EM: the highest printed posterior, the first on ties; where several lines print the same highest
    posterior, the taxon PREFIX.EM.reads2Taxon names for the read decides among them (classify chose from the unrounded posteriors)"""
    out = []
    for r, lines in enumerate(em_reads):
        top = max(float(f[13]) for f in lines)
        cand = [k for k, f in enumerate(lines) if float(f[13]) == top]
        named = [k for k in cand if TAXID.search(lines[k][5]).group(1) == r2t[r][1]]
        out.append((named or cand)[0])
    return out


def taxonomy(db_dir):
    parent, rank, name = {}, {}, {}
    for ln in open(os.path.join(db_dir, "taxonomy", "nodes.dmp")):
        f = [x.strip() for x in ln.split("|")]
        if len(f) > 2:
            parent[f[0]], rank[f[0]] = f[1], f[2]
    for ln in open(os.path.join(db_dir, "taxonomy", "names.dmp")):
        f = [x.strip() for x in ln.split("|")]
        if len(f) > 3 and f[3] == "scientific name":
            name[f[0]] = f[1]
    return parent, rank, name


def at_rank(parent, rank, t, level):
    """the node itself or its nearest ancestor of that rank ('no rank' nodes never count), or '0'"""
    while True:
        if rank[t] == level and level != "no rank":
            return t
        if t == "1" or parent[t] == t:
            return "0"
        t = parent[t]


def recompute(prefix, db_dir, T, refit=False):
    """({suffix behind PREFIX: text}, numbers).  With refit: files also holds '.EM-filtered.refit' WITHOUT the last field of every line, and numbers the
    kept reads / entries and, per read with a mapping, the indices of its kept lines."""
    thr = T * 100.0
    raw, em = read_groups(prefix), read_groups(prefix + ".EM")
    assert [[f[:13] for f in g] for g in raw] == [[f[:13] for f in g] for g in em]
    r2t = [ln.split("\t") for ln in open(prefix + ".EM.reads2Taxon").read().splitlines() if ln]
    unmapped = [int(m.group(1)) for m in re.finditer(r"^definedGenomes\t-3\treadsLongEnough_unmapped\t(\d+)\t", open(prefix + ".EM.WIMP").read(), re.M)]
    assert len(unmapped) == 1
    unmapped = unmapped[0]
    # the largest identity of every read, in numeric order, ties in read order, printed as the text of the field
    mx = []
    for r, lines in enumerate(raw):
        k = max(range(len(lines)), key=lambda k: (float(lines[k][12]), -k))
        mx.append((float(lines[k][12]), r, lines[k][12]))
    mx.sort(key=lambda x: (x[0], x[1]))
    files = {".extractedIdentities": "".join(x[2] + "\n" for x in mx)}
    n_le = sum(1 for x in mx if x[0] <= thr)
    # the genomes' medians
    best = best_lines(em, r2t)
    taxon = [TAXID.search(em[r][best[r]][5]).group(1) for r in range(len(em))]
    per = {}
    for r in range(len(em)):
        per.setdefault(taxon[r], []).append(float(em[r][best[r]][12]))
    median = {t: sorted(x)[len(x) // 2] for t, x in per.items()}
    removed = {t for t, m in median.items() if m < thr}
    # the filtered files
    files[".EM-filtered"] = "".join(" ".join(em[r][best[r]]) + "\n" for r in range(len(em)) if taxon[r] not in removed)
    gone = {em[r][0][0] for r in range(len(em)) if taxon[r] in removed}
    assert [x[0] for x in r2t[:len(em)]] == [g[0][0] for g in em]
    files[".EM-filtered.reads2Taxon"] = "".join(x[0] + "\t" + ("0" if k < len(em) and x[0] in gone else x[1]) + "\n" for k, x in enumerate(r2t))
    parent, rank, name = taxonomy(db_dir)
    rows = ["AnalysisLevel\ttaxonID\tName\tAbsolute\tEMFrequency\tPotFrequency"]
    total = unmapped + len(em)
    for level in ("definedGenomes", "species", "genus", "family"):
        dist = {"0": unmapped + len(gone)}
        for r in range(len(em)):
            if taxon[r] not in removed:
                t = taxon[r] if level == "definedGenomes" else at_rank(parent, rank, taxon[r], level)
                dist[t] = dist.get(t, 0) + 1
        order = ["0"] + sorted((t for t in dist if t != "0"), key=lambda t: (-dist[t], t.encode()))
        for t in order:
            rows.append("%s\t%s\t%s\t%d\tNA\t%.15g" % (level, t, "Unclassified" if t == "0" else name[t], dist[t], dist[t] / total))
    files[".EM-filtered.WIMP"] = "\n".join(rows) + "\n"
    numbers = dict(thr=thr, median_all=mx[len(mx) // 2][0], n_le=n_le, n=len(mx), genomes=len(per), genomes_removed=len(removed), reads_removed=len(gone),
                   medians=median, removed=removed, best=best, taxon=taxon)
    if refit:
        kept = [[k for k, f in enumerate(g) if TAXID.search(f[5]).group(1) not in removed] for g in em]
        files[".EM-filtered.refit"] = "".join(" ".join(em[r][k][:13]) + "\n" for r in range(len(em)) for k in kept[r])
        numbers.update(kept=kept, kept_reads=sum(1 for k in kept if k), kept_entries=sum(len(k) for k in kept), lost=sum(1 for k in kept if not k))
    return files, numbers
