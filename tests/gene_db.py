"""A small gene-annotated database for the tests of `classify --genes`: the synthetic DB directory of metamaps_amd/synth.py plus DB_annotations.txt and
DB_proteins.faa.annotated as a `buildDB.pl --annotations` database carries them.  Genes of 300 - 3 000 bp tile 85 % of every contig but one; among them
nested and overlapping genes, one operon-sized gene that contains 30 others, genes without a locus tag or without a protein, one GeneName//GeneLocusTag
on two contigs and one twice on the same contig.  Proteins carry random subsets of the five annotation fields, with blanks behind commas and repeated
values; one protein is in no genome annotation, some genes' proteins are in no protein line.  The lines are shuffled: nothing may rely on file order."""
import os

import numpy as np

ANNOT_HEADER = ["ContigId", "Type", "Start", "Stop", "Strand", "GeneName", "GeneLocusTag", "CDSProteinId", "CDSProduct"]
PROT_HEADER = ["ProteinID", "seed_ortholog", "evalue", "GO_terms", "KEGG_KOs", "BiGG_reactions", "Annotation_tax_scope", "OGs", "COG_cat", "description"]
COG_LETTERS = "DMNOTUVWYZABJKLCEFGHIPQRS"


def make(out_dir, n_genomes=40, genome_len=30_000, seed=7):
    from metamaps_amd import synth
    db = synth.make_db(out_dir, n_genomes=n_genomes, genome_len=genome_len, seed=seed)
    add_annotations(db, seed + 1)
    return db


def _field(rng, pool, p_empty=0.4, k_max=4):
    if rng.random() < p_empty:
        return ""
    v = [pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, k_max + 1)))]
    if rng.random() < 0.3:
        v.append(v[0])                                              # a repeated value
    return (", " if rng.random() < 0.5 else ",").join(v)


def add_annotations(db, seed):
    rng = np.random.default_rng(seed)
    sizes = [s.size for s in db.contig_seqs]
    big = [c for c in np.argsort(sizes)[::-1] if sizes[c] > 5000]
    bare = int(big[3])                                              # a contig without annotations (a large one: reads do map there)
    rows = []

    def gene(c, start, stop, name=None, locus=None, protein=None):
        k = len(rows)
        if protein is None:
            protein = "" if rng.random() < 0.08 else f"WP_{int(rng.integers(0, 1500)):06d}.1"   # proteins shared between genomes; some genes have none
        rows.append([db.contig_ids[c], "CDS" if protein else "tRNA", str(start), str(stop), "+-"[k % 2], f"gene{k}" if name is None else name,
                     ("" if rng.random() < 0.15 else f"LT_{k:05d}") if locus is None else locus, protein, f"product of gene {k}" if k % 9 else ""])

    for c in range(len(sizes)):
        if c == bare or sizes[c] < 2000:
            continue
        pos, first = int(rng.integers(1, 200)), len(rows)
        while pos + 300 < sizes[c]:
            ln = int(rng.integers(300, 701 if c == int(big[0]) else 3001))   # (short genes on the operon's contig: more than 30 of them)
            stop = min(pos + ln - 1, sizes[c])
            gene(c, pos, stop)
            u = rng.random()
            if u < 0.06 and stop - pos > 200:
                gene(c, pos + 50, pos + 150)                        # nested
            elif u < 0.12:
                gene(c, stop - 40, min(stop + 400, sizes[c]))       # overlapping the next
            pos = stop + 1 + int(rng.exponential(0.15 / 0.85 * 1650))
        if c == int(big[0]):                                        # an operon-sized gene that contains 30 others
            inner = rows[first + 2:first + 32]
            assert len(inner) == 30
            gene(c, int(inner[0][2]), int(inner[-1][3]), name="operonA", locus="LT_OPERON")
        if c == int(big[1]):                                        # one group twice on this contig, 60 bp apart (one read overlaps both: counts twice) ...
            a = int(rows[first + 3][2])
            gene(c, a, a + 300, name="rrsA", locus="", protein="WP_900001.1")
            gene(c, a + 360, a + 700, name="rrsA", locus="", protein="WP_900001.1")
    for c in (int(big[1]), int(big[2])):                            # ... and one GeneName//GeneLocusTag on two contigs
        gene(c, 1000, 2500, name="dnaA", locus="LT_SHARED", protein="WP_900002.1")
    order = rng.permutation(len(rows))
    with open(os.path.join(db.dir, "DB_annotations.txt"), "w") as f:
        f.write("\t".join(ANNOT_HEADER) + "\n")
        for i in order:
            f.write("\t".join(rows[int(i)]) + "\n")
        f.write("\n")                                               # an empty line is skipped
    go = [f"GO:{int(x):07d}" for x in rng.integers(1, 99999, size=60)]
    ko = [f"ko:K{int(x):05d}" for x in rng.integers(1, 20000, size=40)]
    bigg = [f"R_{int(x)}" for x in rng.integers(1, 5000, size=20)]
    ogs = [f"COG{int(x):04d}@1|root" for x in rng.integers(1, 5000, size=50)]
    proteins = sorted({r[7] for r in rows if r[7]})
    proteins = [p for p in proteins if rng.random() < 0.85] + ["WP_999999.1"]   # some genes' proteins are not annotated; one annotated protein is in no genome
    with open(os.path.join(db.dir, "DB_proteins.faa.annotated"), "w") as f:
        f.write("\t".join(PROT_HEADER) + "\n")
        for p in [proteins[int(i)] for i in rng.permutation(len(proteins))]:
            f.write("\t".join([p, "511145.b0001", "1e-50", _field(rng, go), _field(rng, ko), _field(rng, bigg, 0.8), "Bacteria", _field(rng, ogs, 0.3),
                               _field(rng, list(COG_LETTERS), 0.3, 2), ""]) + "\n")
    db.bare_contig = db.contig_ids[bare]
    return db
