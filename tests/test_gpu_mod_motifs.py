"""mm_mod_motifs (methylation per sequence motif on the device: metamaps_amd/csrc/mm_motif.hip, mm_motif_core.hpp) through capi.py against the plain
restatement tests/motif_ref.py: the cases of tests/motif_cases.py one by one and all in one call (with and without combined strands), groups of one contig
each against the single call, a repeated call, an empty table, and every refusal with its message."""
import numpy as np
import pytest

import mods_ref
import motif_cases
import motif_ref

pytestmark = pytest.mark.gpu
ROWS, SUMMARY = ("site", "motif", "code", "n_mod", "n_canonical", "n_other", "n_fail"), ("s_contig", "s_motif", "s_code")


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def call(ctx, ref, w, lo=0, hi=None, keys=None, **over):
    keys = sorted(w["table"]) if keys is None else keys
    a = dict(min_coverage=w["min_coverage"], min_frac=w["min_frac"], combine_strands=w["combine"])
    a.update(over)
    return ctx.mod_motifs(ref, lo, len(w["contigs"]) if hi is None else hi, keys, [w["table"].get(k, 1) for k in keys], w["code_base"], w["motifs"], **a)


def lists(got):
    return (list(zip(*(got[k].tolist() for k in ROWS))), [tuple(a) + tuple(b) for a, b in zip(zip(*(got[k].tolist() for k in SUMMARY)), got["sums"].tolist())])


def want_of(w):
    rows, summary = motif_ref.profile(w["contigs"], w["table"], w["code_base"], w["motifs"], w["min_coverage"], w["min_frac"], w["combine"])
    return [(mods_ref.key(c, pos, strand if strand else 1, 0), j, k, a, b, o, f) for c, pos, strand, j, k, a, b, o, f in rows], [tuple(s) for s in summary]


@pytest.fixture(scope="module")
def worlds(ctx):
    """every world with its reference on the device and the restatement's answer: made once, never changed"""
    ws = {w["name"]: w for w in motif_cases.cases()}
    ws["all_in_one"], ws["all_in_one_combined"] = motif_cases.all_in_one(False), motif_cases.all_in_one(True)
    ws["many_units"], ws["many_units_combined"] = motif_cases.many_units(False), motif_cases.many_units(True)   # (thousands of rows: the units' order by the device-wide sort)
    out = {name: (w, ctx.seqset(w["contigs"]), want_of(w)) for name, w in ws.items()}
    yield out
    for _, ref, _ in out.values():
        ref.close()


@pytest.mark.parametrize("name", [c["name"] for c in motif_cases.cases()] + ["all_in_one", "all_in_one_combined", "many_units", "many_units_combined"])
def test_case(ctx, worlds, name):
    w, ref, want = worlds[name]
    assert lists(call(ctx, ref, w)) == want


@pytest.mark.parametrize("name", ["all_in_one", "all_in_one_combined", "three_tiles_boundary"])
def test_groups_of_one_contig_concatenate_to_the_single_call(ctx, worlds, name):
    w, ref, want = worlds[name]
    rows, summary = [], []
    for c in range(len(w["contigs"])):
        r, s = lists(call(ctx, ref, w, c, c + 1))
        rows += r; summary += s
    assert (rows, summary) == want
    mid = len(w["contigs"]) // 2                                    # and two groups of several contigs
    a, b = lists(call(ctx, ref, w, 0, mid)), lists(call(ctx, ref, w, mid, len(w["contigs"])))
    assert (a[0] + b[0], a[1] + b[1]) == want


def test_a_second_call_returns_the_same_arrays(ctx, worlds):
    w, ref, _ = worlds["all_in_one"]
    a, b = call(ctx, ref, w), call(ctx, ref, w)
    assert all(np.array_equal(a[k], b[k]) for k in a) and len(a["site"]) > 100


def test_an_empty_table_and_an_empty_group(ctx, worlds):
    w, ref, _ = worlds["three_contigs_one_tile"]
    got = call(ctx, ref, dict(w, table={}))
    assert len(got["site"]) == 0 and len(got["s_contig"]) == 0 and got["sums"].shape == (0, 5)
    got = call(ctx, ref, w, 1, 1)
    assert len(got["site"]) == 0 and len(got["s_contig"]) == 0


def test_refusals(ctx, worlds):
    from metamaps_amd import capi
    w, ref, _ = worlds["three_contigs_one_tile"]                   # contigs of 10, 10 and 12 bases, codes CCA
    K = mods_ref.key

    def refused(what, **over):
        with pytest.raises(capi.MMError) as e:
            call(ctx, ref, dict(w, **{k: v for k, v in over.items() if k in w}), **{k: v for k, v in over.items() if k not in w})
        assert e.value.status == -1 and "mm_mod_motifs: " + what in str(e.value) and ctx.last_motif_handle is None, (what, str(e.value))

    refused("the keys are not ascending and unique (entry 1)", keys=[K(0, 5, 1, 1), K(0, 4, 1, 1)])
    for key in (K(0, 10, 1, 1), K(3, 0, 1, 1), K(0, 5, 1, 6), K(0, 5, -1, 7)):
        refused("entry 0 names no position of the reference, or no class of the asked codes", keys=[key])
    refused("n_codes is not in [1, 4]", code_base="")
    refused("n_codes is not in [1, 4]", code_base="CCAAC")
    refused("code 1: the base is not one of A C G T", code_base="CN")
    refused("min_coverage is below 1", min_coverage=0)
    refused("min_frac is not in [0, 1]", min_frac=1.5)
    refused("[contig_lo, contig_hi) is no range", hi=4)
    refused("[contig_lo, contig_hi) is no range", lo=2, hi=1)
    refused("n_motifs is not in [1, 8]", motifs=[])
    refused("n_motifs is not in [1, 8]", motifs=[("CG", 0)] * 9)
    refused("motif 1: the length is not in [1, 32]", motifs=[("CG", 0), ("C" * 33, 0)])
    refused("motif 1: the length is not in [1, 32]", motifs=[("CG", 0), ("", 0)])
    refused("motif 0: letter 1 is no set of A C G T", motifs=[([2, 0], 0)])
    refused("motif 0: letter 1 is no set of A C G T", motifs=[([2, 16], 0)])
    refused("motif 2: the modified base is not one letter of A C G T inside the motif", motifs=[("CG", 0), ("AA", 0), ("CNG", 1)])
    refused("motif 0: the modified base is not one letter of A C G T inside the motif", motifs=[("CG", 2)])
    refused("motif 0: the modified base is not one letter of A C G T inside the motif", motifs=[("CG", -1)])
    refused("motif 1: combine_strands needs a motif that is its own reverse complement", motifs=[("CG", 0), ("GGTGA", 4)], combine_strands=True)
