"""mm_em_bootstrap (EM.bootstrap): the read-level Poisson bootstrap of the EM on the device, against mm_em_run, a float64 numpy weighted EM
with the same weights and stop rule, exact identities of the weights, splits of the replicates, and its refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from em_latency import problem                                  # noqa: E402
from test_boot_core import weights_np                           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def long_reads_problem(n_reads=3000, n_taxa=40, n_present=12, seed=3, unmapped_every=0):
    """reads of 1 to 30 mappings (the long-read path of P1b), taxa of more than 512 mappings (several sum items); unmapped_every = k: reads
    0, k, 2k, ... have no mapping, so that a read's index among the mapped reads (the weights' index) is not its index"""
    rng = np.random.default_rng(seed)
    present = rng.choice(n_taxa, size=n_present, replace=False)
    nm = rng.integers(1, 31, size=n_reads)
    nm[rng.random(n_reads) < 0.5] = 1
    if unmapped_every:
        nm[::unmapped_every] = 0
    off = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
    taxon = present[rng.integers(0, n_present, size=int(off[-1]))].astype(np.int32)
    mapq = rng.uniform(0.01, 1.0, len(taxon))
    inv = 1.0 / rng.integers(1000, 9000, size=len(taxon)).astype(np.float64)
    return off, taxon, mapq, inv, n_taxa


# long_reads_some_unmapped: every third read without a mapping.  The exact reference (post_ref.boot_expected, replicates 0 .. 15 of seed 99 from
# its own point estimate) stops after 3 or 4 iterations and stands off both stop thresholds by 0.019 at least in its last two.
PROBLEMS = {"bench_shape": lambda: problem(100_000), "long_reads": long_reads_problem,
            "long_reads_some_unmapped": lambda: long_reads_problem(seed=4, unmapped_every=3)}


def read_weights(off, w_mapped):
    """weights of the mapped reads, in their order -> a weight per read (0 for a read without a mapping)"""
    w = np.zeros(len(off) - 1, dtype=np.int64)
    w[np.diff(off) > 0] = w_mapped
    return w


def np_weighted_em(off, taxon, mapq, inv, T, f0, w, max_iter=10_000):
    """fEM.h:350-361, :578, :606-615 with per-read weights w, the stop rule of :624-639: (f, ll, iterations, stopped)"""
    n = len(off) - 1
    rid = np.repeat(np.arange(n), np.diff(off))
    f = f0.astype(np.float64).copy()
    ll_prev, it = 0.0, 0
    w = w.astype(np.float64)
    while True:
        lik = f[taxon] * inv * mapq
        S = np.zeros(n); np.add.at(S, rid, lik)
        with np.errstate(divide="ignore", invalid="ignore"):
            post = np.where(w[rid] > 0, w[rid] * lik / S[rid], 0.0)
            ll = float(np.sum(np.where(w > 0, w * np.log(S), 0.0)))
        s = np.bincount(taxon, weights=post, minlength=T)
        f = s / s.sum()
        stop = it > 0 and (ll - ll_prev) <= 1 and (1 - ll / ll_prev) < 1e-4
        it += 1
        ll_prev = ll
        if stop or it >= max_iter:
            return f, ll, it, stop


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_unit_weights_equal_the_point_em(ctx, name):
    off, taxon, mapq, inv, T = PROBLEMS[name]()
    e = ctx.em(off, taxon, mapq, inv, T)
    f0 = np.full(T, 1.0 / T)
    f_pt, lls = e.run(f0, max_iter=1000)
    assert 0 < len(lls) < 1000
    n = int(np.count_nonzero(np.diff(off)))
    fb, llb, itb, stb = e.bootstrap(f0, 4, seed=1, weights=np.ones((4, n), dtype=np.uint8), max_iter=1000)
    assert stb.all()
    for r in range(4):
        assert itb[r] == len(lls)
        np.testing.assert_allclose(fb[r], f_pt, rtol=1e-12, atol=1e-300)
        assert abs(llb[r] - lls[-1]) <= 1e-12 * abs(lls[-1])
    e.close()


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_generated_weights_match_numpy(ctx, name):
    off, taxon, mapq, inv, T = PROBLEMS[name]()
    if name == "bench_shape":
        off, taxon, mapq, inv, T = problem(20_000)
    e = ctx.em(off, taxon, mapq, inv, T)
    f_hat, _ = e.run(np.full(T, 1.0 / T), max_iter=1000)
    n, B, seed = int(np.count_nonzero(np.diff(off))), 16, 99
    fb, llb, itb, stb = e.bootstrap(f_hat, B, seed=seed)
    for r in range(B):
        w = read_weights(off, weights_np(np.uint64(seed), np.uint64(r), np.arange(n, dtype=np.uint64)))
        f, ll, it, stop = np_weighted_em(off, taxon, mapq, inv, T, f_hat, w)
        assert itb[r] == it and stb[r] == stop, (r, itb[r], it)
        np.testing.assert_allclose(fb[r], f, rtol=0, atol=1e-9)
        assert abs(llb[r] - ll) <= 1e-12 * abs(ll)
    e.close()


def test_zero_one_weights_drop_reads_and_twos_duplicate_them(ctx):
    off, taxon, mapq, inv, T = long_reads_problem()
    n = len(off) - 1
    f0 = np.full(T, 1.0 / T)
    e = ctx.em(off, taxon, mapq, inv, T)
    rng = np.random.default_rng(8)
    keep = rng.random(n) < 0.7
    fb, llb, itb, _ = e.bootstrap(f0, 1, seed=1, weights=keep.astype(np.uint8)[None, :])
    idx = [np.arange(off[i], off[i + 1]) for i in range(n) if keep[i]]
    sel = np.concatenate(idx)
    off2 = np.concatenate([[0], np.cumsum([len(x) for x in idx])]).astype(np.int64)
    e2 = ctx.em(off2, taxon[sel], mapq[sel], inv[sel], T)
    f2, lls2 = e2.run(f0, max_iter=10_000)
    assert itb[0] == len(lls2)
    np.testing.assert_allclose(fb[0], f2, rtol=1e-12, atol=1e-300)
    assert abs(llb[0] - lls2[-1]) <= 1e-12 * abs(lls2[-1])
    e2.close()
    # every read twice
    fb2, llb2, itb2, _ = e.bootstrap(f0, 1, seed=1, weights=np.full((1, n), 2, dtype=np.uint8))
    dup = np.concatenate([np.concatenate([np.arange(off[i], off[i + 1])] * 2) for i in range(n)])
    off3 = np.concatenate([[0], np.cumsum(np.repeat(np.diff(off), 2))]).astype(np.int64)
    e3 = ctx.em(off3, taxon[dup], mapq[dup], inv[dup], T)
    f3, lls3 = e3.run(f0, max_iter=10_000)
    np.testing.assert_allclose(fb2[0], f3, rtol=1e-12, atol=1e-300)
    assert itb2[0] == len(lls3)
    e3.close(); e.close()


def test_splits_and_seeds(ctx):
    off, taxon, mapq, inv, T = long_reads_problem(seed=11)
    e = ctx.em(off, taxon, mapq, inv, T)
    f_hat, _ = e.run(np.full(T, 1.0 / T), max_iter=1000)
    whole = e.bootstrap(f_hat, 12, seed=5)
    a = e.bootstrap(f_hat, 5, seed=5, rep0=0)
    b = e.bootstrap(f_hat, 7, seed=5, rep0=5)
    for k in range(4):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]]))
    again = e.bootstrap(f_hat, 12, seed=5)
    for k in range(4):
        assert np.array_equal(whole[k], again[k])
    other = e.bootstrap(f_hat, 12, seed=6)
    assert not np.array_equal(whole[0], other[0])
    # a tile boundary (64 replicates) inside the split
    big = e.bootstrap(f_hat, 70, seed=5, max_iter=3)
    c = e.bootstrap(f_hat, 60, seed=5, max_iter=3)
    d = e.bootstrap(f_hat, 10, seed=5, rep0=60, max_iter=3)
    assert np.array_equal(big[0], np.concatenate([c[0], d[0]])) and np.array_equal(big[1], np.concatenate([c[1], d[1]]))
    e.close()


def test_refusals(ctx):
    from metamaps_amd import capi
    off, taxon, mapq, inv, T = long_reads_problem(n_reads=500)
    e = ctx.em(off, taxon, mapq, inv, T)
    f0 = np.full(T, 1.0 / T)
    for n_rep in (0, -3):
        with pytest.raises(capi.MMError) as ei:
            e.bootstrap(f0, n_rep, seed=1)
        assert ei.value.status == -1
    with pytest.raises(capi.MMError) as ei:
        e.bootstrap(f0, 10, seed=1, rep0=2**31 - 5)
    assert ei.value.status == -1
    e.close()
    # post_b beyond the device: 8 * n_entries * n_rep bytes > 288 GB
    off, taxon, mapq, inv, T = problem(250_000, n_taxa=4, n_present=2)
    e = ctx.em(off, taxon, mapq, inv, T)
    with pytest.raises(capi.MMError) as ei:
        e.bootstrap(np.full(T, 0.25), 40_000_000, seed=1)
    assert ei.value.status in (-3, -5)
    e.close()
