"""mm_mapping_edit_distances: the exact edit distance and the real first and last contig coordinate of every record of a mapping, the jobs made on the
device from the records by the window and cap rules (metamaps_amd/csrc/mm_edit.hip), against the naive dynamic programme (tests/edit_ref.py: record).
A few 20 kb contigs; 40 reads of 2-3 kb cut from them at 0 %, 5 % and 12 % errors on both strands, some within 100 bases of a contig's end so that the
window is clipped; mapped with mm_map_batch.  Every comparison is exact."""
import numpy as np
import pytest

import edit_cases
import edit_ref

pytestmark = pytest.mark.gpu
K, W, PI = 16, 10, 80.0


@pytest.fixture(scope="module")
def world():
    from metamaps_amd import capi, synth
    rng = np.random.default_rng(21)
    ctx = capi.Context(0)
    contigs = [synth.random_genome(rng, 20_000 + 37 * c).tobytes() for c in range(4)]
    reads, truth = [], []
    for r in range(40):
        c, L = r % 4, int(rng.integers(2000, 3001))
        C = len(contigs[c])
        start = [int(rng.integers(0, 100)), C - L - int(rng.integers(0, 100))][r % 2] if r % 10 < 2 else int(rng.integers(200, C - L - 200))
        rate, strand = (0.0, 0.05, 0.12)[r % 3], 1 if (r // 3) % 2 == 0 else -1
        piece = np.frombuffer(contigs[c][start:start + L], dtype=np.uint8)
        seq = synth.mutate(rng, piece, sub=rate / 3, ins=rate / 3, dele=rate / 3).tobytes()
        reads.append(edit_cases.stored(seq, strand))
        truth.append((c, start, L, rate, strand))
    ref, rd = ctx.seqset(contigs), ctx.seqset(reads)
    idx = ctx.index(ref, K, W)
    M = ctx.map_batch(idx, rd, K, W, pi=PI)
    off, rec = M.fetch()
    rec = rec.copy()
    dist, first, last = ctx.mapping_edit_distances(M, rd, ref, PI, len(rec))
    out = dict(ctx=ctx, contigs=contigs, reads=reads, truth=truth, rec=rec, got=list(zip(dist.tolist(), first.tolist(), last.tolist())), ref=ref, rd=rd)
    yield out
    M.close(); idx.close(); ref.close(); rd.close(); ctx.close()


def test_every_record_against_the_reference(world):
    rec = world["rec"]
    assert len(rec) >= 30 and len(set(rec["read"].tolist())) >= 30 and {-1, 1} <= set(rec["strand"].tolist())
    clipped = 0
    for r, got in zip(rec, world["got"]):
        read, contig = world["reads"][r["read"]], world["contigs"][r["ref_contig"]]
        want = edit_ref.record(read, int(r["strand"]), contig, int(r["ref_start"]), PI)
        assert got == ((-1, -1, -1) if want is None else want), (r, got, want)
        ws, we = edit_ref.window(int(r["ref_start"]), len(read), len(contig))
        clipped += ws == 0 or we == len(contig)
    assert clipped >= 4                                            # windows cut at a contig's end
    assert sum(g[0] > 100 for g in world["got"]) >= 10


def test_error_free_reads_come_back_at_their_locus(world):
    seen = 0
    for r, got in zip(world["rec"], world["got"]):
        c, start, L, rate, strand = world["truth"][r["read"]]
        if rate == 0.0 and r["ref_contig"] == c:
            assert got == (0, start, start + L - 1) and r["strand"] == strand
            seen += 1
    assert seen >= 10


def test_a_random_read_forced_onto_a_contig_is_not_aligned(world):
    ctx, rng = world["ctx"], np.random.default_rng(3)
    L = 2500
    rd = ctx.seqset([edit_cases.dna(rng, L)])
    ws, we = edit_ref.window(5000, L, len(world["contigs"][1]))
    try:
        dist, a, b = ctx.edit_infix(rd, world["ref"], read=[0], strand=[1], contig=[1], ws=[ws], we=[we], max_dist=[edit_ref.cap(L, PI)])
    finally:
        rd.close()
    assert edit_ref.record(rd_bytes := edit_cases.dna(np.random.default_rng(3), L), 1, world["contigs"][1], 5000, PI) is None and len(rd_bytes) == L
    assert (int(dist[0]), int(a[0]), int(b[0])) == (-1, -1, -1)
