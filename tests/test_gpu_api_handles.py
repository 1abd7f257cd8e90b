"""Every entry point of libmetamaps_hip.so that hands back a new handle leaves *out NULL when it fails (include/metamaps_hip.h, opening comment).
Each case presets *out to a non-null sentinel, provokes one error that the library's host code refuses before any launch (the MM_REQUIRE named
beside the case), and then makes a correct call of the same entry point on the same context.  The world is two 200-base sequences.
Left out, for want of an error between the null-argument check and the first launch: mm_seqset_create (nothing of it can fail but an allocation)
and mm_gzip_open (mm::gzip_open takes every chunk and segment size)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, W = 16, 5
SENTINEL = 0xDEAD0


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class World:
    def __init__(self):
        from metamaps_amd import capi
        self.capi, self.L = capi, capi.lib()
        self.ctx = capi.Context(0)
        rng = np.random.default_rng(7)
        self.seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=200)) for _ in range(2)]
        self.set = self.ctx.seqset(self.seqs)                     # uploaded
        self.staged = C.c_void_p()                                # created, never uploaded
        assert self.L.mm_seqset_create(self.ctx.h, C.byref(self.staged)) == 0 and self.staged.value
        assert self.L.mm_seqset_add(self.staged, self.seqs[0], 200) == 0
        self.idx = self.ctx.index(self.set, K, W)
        self.params = capi.MapParams(K, W, 80.0, 1000)
        self.bad_k = capi.MapParams(65, W, 80.0, 1000)
        off = np.array([0, 1, 1, 2], dtype=np.int64)              # a mapping of THREE reads, from host arrays
        rec = np.zeros(2, dtype=capi.RECORD_DTYPE)
        rec["read"] = [0, 2]; rec["sketch"] = 20; rec["shared"] = 10; rec["strand"] = 1
        self.three = capi.Mapping.from_parts(self.ctx, np.array([200, 200, 200], dtype=np.int32), [(off, rec)], [0], K, W)
        self.keep = []                                            # arrays a call reads

    def close(self):
        self.three.close(); self.idx.close(); self.set.close()
        self.L.mm_seqset_destroy(self.staged)
        self.ctx.close()

    def refused(self, call, n_out=1):
        """call(out pointers ...) -> status, with every *out preset: status, message and *out as the header promises"""
        outs = [C.c_void_p(SENTINEL + i) for i in range(n_out)]
        st = call(*[C.byref(o) for o in outs])
        assert st != 0
        assert self.L.mm_last_error(self.ctx.h)
        for o in outs:
            assert o.value is None                                 # (ctypes' NULL)

    def made(self, call, destroy, n_out=1):
        outs = [C.c_void_p(SENTINEL + i) for i in range(n_out)]
        st = call(*[C.byref(o) for o in outs])
        assert st == 0, self.L.mm_last_error(self.ctx.h)
        for o, d in zip(outs, destroy):
            assert o.value not in (None, SENTINEL, SENTINEL + 1)
            d(o)


@pytest.fixture(scope="module")
def w():
    world = World()
    yield world
    world.close()


def test_seqset_load_of_a_missing_file(w, tmp_path):             # seqset_load: the file cannot be opened
    good = str(tmp_path / "two.seqset")
    w.set.save(good)
    w.refused(lambda o: w.L.mm_seqset_load(w.ctx.h, str(tmp_path / "none.seqset").encode(), o))
    w.made(lambda o: w.L.mm_seqset_load(w.ctx.h, good.encode(), o), [w.L.mm_seqset_destroy])


def test_seqset_slice_beyond_the_set(w):                          # seqset_slice: "slice out of range"
    w.refused(lambda o: w.L.mm_seqset_slice(w.ctx.h, w.set.h, 1, 2, o))
    w.made(lambda o: w.L.mm_seqset_slice(w.ctx.h, w.set.h, 1, 1, o), [w.L.mm_seqset_destroy])


def test_seqset_concat_of_a_set_not_uploaded(w):                  # seqset_concat: "sequence set not uploaded"
    bad = (C.c_void_p * 2)(w.set.h, w.staged)
    good = (C.c_void_p * 2)(w.set.h, w.set.h)
    w.refused(lambda o: w.L.mm_seqset_concat(w.ctx.h, bad, 2, o))
    w.made(lambda o: w.L.mm_seqset_concat(w.ctx.h, good, 2, o), [w.L.mm_seqset_destroy])


def test_seqset_hpc_of_a_set_not_uploaded(w):                     # seqset_hpc: "sequence set not uploaded"; set and map are let go together
    w.refused(lambda o, m: w.L.mm_seqset_hpc(w.ctx.h, w.staged, o, m), n_out=2)
    w.made(lambda o, m: w.L.mm_seqset_hpc(w.ctx.h, w.set.h, o, m), [w.L.mm_seqset_destroy, w.L.mm_hpc_map_destroy], n_out=2)


def test_synth_sets_with_bad_parameters(w):                       # "bad synthetic reference / community / read parameters"
    capi = w.capi
    ref_ok = dict(seed=3, n_species=8, strains_per_species=2, genome_len=200_000, strain_divergence=0.02, genus_divergence=0.2)
    p_bad, p_ok = capi.SynthRefParams(**dict(ref_ok, n_species=0)), capi.SynthRefParams(**ref_ok)
    w.refused(lambda o: w.L.mm_synth_reference(w.ctx.h, C.byref(p_bad), o))
    ref = C.c_void_p()
    assert w.L.mm_synth_reference(w.ctx.h, C.byref(p_ok), C.byref(ref)) == 0 and ref.value
    com_ok = dict(seed=29, n_genomes=24, n_species=8, n_genera=3, median_len=200_000.0, sigma_len=0.5, min_len=20_000, max_len=500_000,
                  strain_div_min=0.001, strain_div_max=0.05, genus_div_min=0.15, genus_div_max=0.25, strain_indel_events=6,
                  human_contigs=2, human_bases=3_000_000, repeat_fraction=0.45, n_fraction=0.01, n_repeat_families=12, total_bases_target=0)
    c_bad, c_ok = capi.SynthCommunityParams(**dict(com_ok, n_genomes=0)), capi.SynthCommunityParams(**com_ok)
    genome = np.zeros(26, dtype=np.int32)
    w.refused(lambda o: w.L.mm_synth_community(w.ctx.h, C.byref(c_bad), o, vp(genome)))
    w.made(lambda o: w.L.mm_synth_community(w.ctx.h, C.byref(c_ok), o, vp(genome)), [w.L.mm_seqset_destroy])
    rd_ok = dict(seed=4, n_reads=20, read_len=9000, sub_rate=0.04, ins_rate=0.03, del_rate=0.05, frac_random=0.05, n_abundant=4)
    r_bad, r_ok = capi.SynthReadParams(**dict(rd_ok, n_reads=0)), capi.SynthReadParams(**rd_ok)
    truth = np.zeros(20, dtype=np.int32)
    try:
        w.refused(lambda o: w.L.mm_synth_reads(w.ctx.h, ref, C.byref(r_bad), o, vp(truth)))
        w.made(lambda o: w.L.mm_synth_reads(w.ctx.h, ref, C.byref(r_ok), o, vp(truth)), [w.L.mm_seqset_destroy])
    finally:
        w.L.mm_seqset_destroy(ref)


def test_index_build_with_k_out_of_range(w):                      # run_minimizers: "k must be in [1,64]"
    w.refused(lambda o: w.L.mm_index_build(w.ctx.h, w.set.h, 65, W, o))
    w.made(lambda o: w.L.mm_index_build(w.ctx.h, w.set.h, K, W, o), [w.L.mm_index_destroy])


def test_index_load_of_a_missing_file(w, tmp_path):               # index_load: "cannot open ..."
    good = str(tmp_path / "two.idx")
    w.idx.save(good)
    w.refused(lambda o: w.L.mm_index_load(w.ctx.h, str(tmp_path / "none.idx").encode(), o))
    w.made(lambda o: w.L.mm_index_load(w.ctx.h, good.encode(), o), [w.L.mm_index_destroy])


def test_map_batch_with_another_k_than_the_index(w):              # MapRun::begin: "index was built with different k / window size"
    cb = w.capi.SEED_STAGE_CB(lambda _user, _stage: None)
    w.refused(lambda o: w.L.mm_map_batch(w.ctx.h, w.idx.h, w.set.h, C.byref(w.bad_k), o))
    w.made(lambda o: w.L.mm_map_batch(w.ctx.h, w.idx.h, w.set.h, C.byref(w.params), o), [w.L.mm_mapping_destroy])
    w.refused(lambda o: w.L.mm_map_batch_phased(w.ctx.h, w.idx.h, w.set.h, C.byref(w.bad_k), cb, None, o))
    w.made(lambda o: w.L.mm_map_batch_phased(w.ctx.h, w.idx.h, w.set.h, C.byref(w.params), cb, None, o), [w.L.mm_mapping_destroy])


def test_sketch_batch_with_k_out_of_range(w):                     # run_minimizers: "k must be in [1,64]" (a sketch needs no index)
    w.refused(lambda o: w.L.mm_sketch_batch(w.ctx.h, w.set.h, C.byref(w.bad_k), o))
    w.made(lambda o: w.L.mm_sketch_batch(w.ctx.h, w.set.h, C.byref(w.params), o), [w.L.mm_mapping_destroy])


def test_map_batch_reusing_a_released_donor(w):                   # mm_map_batch_reusing: "the donor mapping has released its intermediates"
    donor = w.ctx.sketch_batch(w.set, K, W)
    try:
        w.made(lambda o: w.L.mm_map_batch_reusing(w.ctx.h, w.idx.h, w.set.h, C.byref(w.params), donor.h, o), [w.L.mm_mapping_destroy])
        donor.release_intermediates()
        w.refused(lambda o: w.L.mm_map_batch_reusing(w.ctx.h, w.idx.h, w.set.h, C.byref(w.params), donor.h, o))
        w.made(lambda o: w.L.mm_map_batch(w.ctx.h, w.idx.h, w.set.h, C.byref(w.params), o), [w.L.mm_mapping_destroy])
    finally:
        donor.close()


def test_mapping_concat_of_a_sketch(w):                           # mapping_concat: "a part holds no records"
    sketch = w.ctx.sketch_batch(w.set, K, W)
    two = w.ctx.map_batch(w.idx, w.set, K, W)
    base = np.zeros(2, dtype=np.int32)
    try:
        bad, good = (C.c_void_p * 2)(two.h, sketch.h), (C.c_void_p * 2)(two.h, two.h)
        w.refused(lambda o: w.L.mm_mapping_concat(w.ctx.h, bad, vp(base), 2, o))
        w.made(lambda o: w.L.mm_mapping_concat(w.ctx.h, good, vp(base), 2, o), [w.L.mm_mapping_destroy])
    finally:
        sketch.close(); two.close()


def test_em_create_with_a_taxon_out_of_range(w):                  # em_create / em_create_from_mapping: "taxon index out of range"
    off = np.array([0, 1, 2], dtype=np.int64)
    q, inv = np.array([0.5, 0.5]), np.array([1.0, 1.0])
    bad, good = np.array([0, 3], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    w.refused(lambda o: w.L.mm_em_create(w.ctx.h, 2, vp(off), vp(bad), vp(q), vp(inv), 2, o))
    w.made(lambda o: w.L.mm_em_create(w.ctx.h, 2, vp(off), vp(good), vp(q), vp(inv), 2, o), [w.L.mm_em_destroy])
    clen = np.array([200], dtype=np.int32)
    c_bad, c_good = np.array([2], dtype=np.int32), np.array([1], dtype=np.int32)
    w.refused(lambda o: w.L.mm_em_create_from_mapping(w.ctx.h, w.three.h, vp(c_bad), vp(clen), 1, 2, o))
    w.made(lambda o: w.L.mm_em_create_from_mapping(w.ctx.h, w.three.h, vp(c_good), vp(clen), 1, 2, o), [w.L.mm_em_destroy])


def test_edit_infix_align_with_a_negative_job_count(w):           # require_jobs: "a negative number of jobs, or 2^31 or more"
    w.refused(lambda o: w.L.mm_edit_infix_align(w.ctx.h, w.set.h, w.set.h, -1, None, None, None, None, None, None, o))
    one = [np.array([v], dtype=t) for v, t in ((0, np.int32), (1, np.int32), (1, np.int32), (20, np.int64), (120, np.int64), (200, np.int32))]
    w.made(lambda o: w.L.mm_edit_infix_align(w.ctx.h, w.set.h, w.set.h, 1, *[vp(a) for a in one], o), [w.L.mm_alignment_destroy])


def test_mapping_align_with_another_read_set(w):                  # edit_mapping_check: "the read set is not the one that was mapped"
    w.refused(lambda o: w.L.mm_mapping_align(w.ctx.h, w.three.h, w.set.h, w.set.h, 80.0, o))
    two = w.ctx.map_batch(w.idx, w.set, K, W)                     # (of the set's own two reads, both below min_read_len: no records, nothing to align)
    try:
        w.made(lambda o: w.L.mm_mapping_align(w.ctx.h, two.h, w.set.h, w.set.h, 80.0, o), [w.L.mm_alignment_destroy])
    finally:
        two.close()
