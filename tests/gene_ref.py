"""The gene-level analysis of DESIGN.md section 4 ("Gene-level analysis") restated in Python, for the tests of mm_gene_core.hpp, mm_gene_overlap,
host/gene_annot.hpp and `classify --genes`.  Two restatements:
  overlap / overlap_slow   arrays in, arrays out — what mm_gene_overlap computes: all-pairs overlap per contig (Start < e and s <= Stop), counts and
                           identities pooled per gene group, the median = the element of rank (n-1)//2 in ascending order, per-read feature sets
  recompute                text in, text out — every file `classify --genes` writes, from PREFIX.EM and the two annotation tables of the DB directory
Nothing here shares code with the product."""
import os

import numpy as np

TYPES = (("GO_terms", "GO"), ("KEGG_KOs", "KEGG"), ("BiGG_reactions", "BiGG"), ("OGs", "OG"), ("COG_cat", "COG"))
COG = {"D": "Cell cycle control, cell division, chromosome partitioning", "M": "Cell wall/membrane/envelope biogenesis", "N": "Cell motility",
       "O": "Post-translational modification, protein turnover, and chaperones", "T": "Signal transduction mechanisms",
       "U": "Intracellular trafficking, secretion, and vesicular transport", "V": "Defense mechanisms", "W": "Extracellular structures", "Y": "Nuclear structure",
       "Z": "Cytoskeleton", "A": "RNA processing and modification", "B": "Chromatin structure and dynamics", "J": "Translation, ribosomal structure and biogenesis",
       "K": "Transcription", "L": "Replication, recombination and repair", "C": "Energy production and conversion", "E": "Amino acid transport and metabolism",
       "F": "Nucleotide transport and metabolism", "G": "Carbohydrate transport and metabolism", "H": "Coenzyme transport and metabolism",
       "I": "Lipid transport and metabolism", "P": "Inorganic ion transport and metabolism", "Q": "Secondary metabolites biosynthesis, transport, and catabolism",
       "R": "General function prediction only", "S": "Function unknown"}


def all_pairs(off, gs, ge, mc, ms, me, chunk=4096):
    """(mapping, gene) of every overlap, by comparing every mapping of a contig with every gene of it"""
    off, gs, ge, mc, ms, me = (np.asarray(a, dtype=np.int64) for a in (off, gs, ge, mc, ms, me))
    pm, pg = [], []
    order = np.argsort(mc, kind="stable")
    bounds = np.searchsorted(mc[order], np.arange(len(off)))
    for c in range(len(off) - 1):
        a, b = off[c], off[c + 1]
        idx = order[bounds[c]:bounds[c + 1]]
        if b == a or len(idx) == 0:
            continue
        for i in range(0, len(idx), chunk):
            sub = idx[i:i + chunk]
            hit = (gs[a:b][None, :] < me[sub][:, None]) & (ms[sub][:, None] <= ge[a:b][None, :])
            r, k = np.nonzero(hit)
            pm.append(sub[r]); pg.append(k + a)
    if not pm:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(pm), np.concatenate(pg)


def overlap(off, gs, ge, gg, n_groups, foff, feat, n_feats, mc, ms, me, mi):
    """(group_reads, group_median with NaN for empty groups, feat_reads, mappings on contigs with genes)"""
    off, gg, foff, feat, mc = (np.asarray(a, dtype=np.int64) for a in (off, gg, foff, feat, mc))
    mi = np.asarray(mi, dtype=np.float64)
    pm, pg = all_pairs(off, gs, ge, mc, ms, me)
    grp = gg[pg]
    reads = np.bincount(grp, minlength=n_groups).astype(np.int64)
    median = np.full(n_groups, np.nan)
    order = np.lexsort((mi[pm], grp))
    first = np.concatenate([[0], np.cumsum(reads)])
    has = reads > 0
    median[has] = mi[pm][order][(first[:-1] + (reads - 1) // 2)[has]]
    n_f = foff[grp + 1] - foff[grp]
    rep_m = np.repeat(pm, n_f)
    at = np.repeat(foff[grp], n_f) + (np.arange(int(n_f.sum())) - np.repeat(np.cumsum(n_f) - n_f, n_f))
    pairs = np.unique(rep_m * max(n_feats, 1) + feat[at]) if len(at) else np.zeros(0, dtype=np.int64)   # a (mapping, feature) once
    feats = np.bincount(pairs % max(n_feats, 1), minlength=n_feats).astype(np.int64)
    on = int(np.count_nonzero((off[mc + 1] > off[mc]))) if len(mc) else 0
    return reads, median, feats, on


def overlap_slow(off, gs, ge, gg, n_groups, foff, feat, n_feats, mc, ms, me, mi):
    """the same by plain loops (small inputs): what `overlap` is held against"""
    reads, idents, feats, on = [0] * n_groups, [[] for _ in range(n_groups)], [0] * n_feats, 0
    for m in range(len(mc)):
        a, b = int(off[mc[m]]), int(off[mc[m] + 1])
        on += b > a
        mine = set()
        for j in range(a, b):
            if gs[j] < me[m] and ms[m] <= ge[j]:
                g = int(gg[j])
                reads[g] += 1
                idents[g].append(float(mi[m]))
                mine.update(int(f) for f in feat[foff[g]:foff[g + 1]])
        for f in mine:
            feats[f] += 1
    median = [sorted(x)[(len(x) - 1) // 2] if x else float("nan") for x in idents]
    return np.array(reads, dtype=np.int64), np.array(median), np.array(feats, dtype=np.int64), on


# ---- text level

def best_mappings(prefix):
    """per read with a mapping (contig, start, stop, identity) of its best mapping as printed: the line with the highest posterior (field 14), the first
    on ties; where several lines of a read print the same highest posterior (six decimals), the contig that PREFIX.EM.lengthAndIdentitiesPerMappingUnit
    names for the read decides among them — that file carries the best mapping classify itself chose from the unrounded posteriors"""
    li = [ln.split("\t")[1] for ln in open(prefix + ".EM.lengthAndIdentitiesPerMappingUnit").read().splitlines()[1:]]
    reads, cur = [], None
    for ln in open(prefix + ".EM"):
        f = ln.rstrip("\n").split(" ")
        if len(f) < 14:
            continue
        if f[0] != cur:
            cur = f[0]
            reads.append([])
        reads[-1].append(f)
    out = []
    for r, lines in enumerate(reads):
        top = max(float(f[13]) for f in lines)
        cand = [f for f in lines if float(f[13]) == top]
        if len(cand) > 1 and any(f[5] == li[r] for f in cand):
            cand = [f for f in cand if f[5] == li[r]]
        f = cand[0]
        assert int(f[7]) <= int(f[8])
        out.append((f[5], int(f[7]), int(f[8]), float(f[9]) / 100))
    return out


def _rows(path):
    with open(path) as fh:
        header = fh.readline().rstrip("\n").split("\t")
        for ln in fh:
            ln = ln.rstrip("\n")
            if ln:
                yield header, ln.split("\t")


def recompute(prefix, db_dir):
    """{suffix behind PREFIX.EM: text} of the files `classify --genes` writes, and the numbers of its messages"""
    return recompute_from_best(best_mappings(prefix), db_dir)


def recompute_from_best(best, db_dir):
    """the same from the reads' best mappings [(contig ID, start, stop, identity)]"""
    relevant = {b[0] for b in best}
    genes, groups, order, known = {}, {}, [], set()
    for header, f in _rows(os.path.join(db_dir, "DB_annotations.txt")):
        assert header[0] == "ContigId"
        row = dict(zip(header, f))
        known.add(row["CDSProteinId"])
        if f[0] not in relevant:
            continue
        gid = row["GeneName"] + "//" + row["GeneLocusTag"]
        if gid not in groups:
            order.append(gid)
        groups[gid] = (row["GeneName"], row["GeneLocusTag"], row["CDSProteinId"], row["CDSProduct"])
        genes.setdefault(f[0], []).append((int(row["Start"]), int(row["Stop"]), gid))
    wanted = {g[2] for g in groups.values() if g[2]}
    annot, n_lines, n_absent = {}, 0, 0
    for header, f in _rows(os.path.join(db_dir, "DB_proteins.faa.annotated")):
        assert len(f) == len(header)
        row = dict(zip(header, f))
        n_lines += 1
        n_absent += row["ProteinID"] not in known
        if row["ProteinID"] not in wanted:
            continue
        assert row["ProteinID"] not in annot
        annot[row["ProteinID"]] = {t: {v for v in "".join(row[col].split()).split(",") if v} for col, t in TYPES}
    n_reads, idents, support, on = {}, {}, {t: {} for _, t in TYPES}, 0
    for contig, s, e, ident in best:
        on += contig in genes
        mine = set()
        for start, stop, gid in genes.get(contig, ()):
            if start < e and s <= stop:
                n_reads[gid] = n_reads.get(gid, 0) + 1
                idents.setdefault(gid, []).append(ident)
                for t, vals in annot.get(groups[gid][2], {}).items():
                    mine.update((t, v) for v in vals)
        for t, v in mine:
            support[t][v] = support[t].get(v, 0) + 1
    files = {}
    rows = ["GeneName\tGeneLocusTag\tProteinId\tProduct\tnReads\tmedianIdentity"]
    for gid in order:
        if gid in n_reads:
            x = sorted(idents[gid])
            rows.append("\t".join(groups[gid]) + "\t%d\t%.15g" % (n_reads[gid], x[(len(x) - 1) // 2]))
    files[".geneLevelAnalysis"] = "\n".join(rows) + "\n"
    for _, t in TYPES:
        if support[t]:
            rows = ["Feature\tSupportByReads\tSupportByReadsProportionTotalReads" + ("\tFeatureLong" if t == "COG" else "")]
            for v in sorted(support[t], key=lambda v: v.encode()):
                rows.append("%s\t%d\t%.15g" % (v, support[t][v], support[t][v] / len(best)) + ("\t" + COG[v] if t == "COG" else ""))
            files[".proteins." + t] = "\n".join(rows) + "\n"
    found = {groups[g][2] for g in n_reads if groups[g][2]}
    stats = {"relevant": len(relevant), "annotated": len(genes), "reads": len(best), "on": on, "genes": len(n_reads), "proteins": len(found),
             "annotated_proteins": sum(1 for p in found if any(annot.get(p, {}).values())), "protein_lines": n_lines, "absent": n_absent}
    return files, stats
