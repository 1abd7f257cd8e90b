"""mm_prims.hpp's with_scratch through real rocprim calls: the smallest sorts and scans the library makes — mm_ident_filter on one read with one entry,
mm_gene_overlap on one mapping over one gene, where a scratch size near zero would show as a sort that did not run — against tests/ident_ref.py and
tests/gene_ref.py, on a fresh context and again behind a call of 70 000 reads (mappings) on the same context, whose freed scratch blocks the small
calls are then served from.  Equality is exact."""
import numpy as np
import pytest

import gene_ref
import ident_ref

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx_own():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


IDENT_ONE = ([0, 1], [0], [85.5], [0], 1, 80.0)
GENE_ONE = ([0, 1], [10], [20], [0], 1, [0, 1], [0], 1, [0], [12], [15], [0.875])


def check_small(ctx, ident_want, gene_want):
    idn = ctx.ident_filter(*IDENT_ONE)
    ident_ref.same(idn, ident_want)
    assert idn["sorted_max"].tolist() == [85.5] and idn["taxon_median"].tolist() == [85.5] and idn["entry_src"].tolist() == [0]
    got = ctx.gene_overlap(*GENE_ONE)
    assert np.array_equal(got[0], gene_want[0]) and np.array_equal(got[1], gene_want[1], equal_nan=True)
    assert np.array_equal(got[2], gene_want[2]) and got[3] == gene_want[3]
    assert got[0].tolist() == [1] and got[1].tolist() == [0.875] and got[2].tolist() == [1]


def test_smallest_sorts_on_a_fresh_context_and_behind_70000(ctx_own):
    ctx = ctx_own
    ident_want = ident_ref.filter_arrays(*IDENT_ONE)
    gene_want = gene_ref.overlap(*GENE_ONE)
    check_small(ctx, ident_want, gene_want)
    rng = np.random.default_rng(71)
    n = 70_000
    big = ctx.ident_filter(np.arange(n + 1), rng.integers(0, 50, size=n), rng.integers(6000, 10001, size=n) / 100.0, np.arange(n), 50, 85.0)
    assert len(big["sorted_max"]) == n and big["taxon_reads"].sum() == n and np.all(np.diff(big["sorted_max"]) >= 0)
    gs = 100 * np.arange(1000)
    ms = rng.integers(0, 100_000, size=n)
    bigg = ctx.gene_overlap([0, 1000], gs, gs + 50, np.arange(1000), 1000, np.arange(1001), np.arange(1000) % 9, 9,
                            np.zeros(n, dtype=np.int32), ms, ms + 60, rng.integers(70, 101, size=n) / 100.0)
    assert bigg[3] == n and n // 2 < bigg[0].sum() < 2 * n
    check_small(ctx, ident_want, gene_want)
