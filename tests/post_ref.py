"""References for the K8 / K9 arithmetic (metamaps_amd/csrc/mm_post_core.hpp, mm_post.hip), for tests/test_post_core.py and
tests/test_gpu_post_edges.py: the exact binomial mass (mpmath, 60 digits), the float64 restatement of the read's success probability and of the
6-digit text round trip, the scale S of the binomial formula's error, and a float64 host EM with exact sums (math.fsum) and the reference's
order of products, with optional per-read weights (the bootstrap of mm_boot.hip; tests/boot_cases.py, tests/test_gpu_boot_edges.py).  Nothing
here touches the device or the library."""
import math

import mpmath
import numpy as np

DBL_MIN = 2.2250738585072014e-308
ULP = 2.0 ** -52
mpmath.mp.dps = 60


def text6(v: float) -> float:
    """what std::stod returns for the "%g" text of v; 0 where it throws (a denormal), fEM.h:269-275"""
    r = float("%g" % v)
    return 0.0 if 0 < abs(r) < DBL_MIN else r


def identity(shared: int, s: int, k: int) -> float:
    """the 6-digit identity of a record as a fraction: float math of map_stats.hpp:44, computeMap.hpp:406,411, the text, / 100 (mapWrap.h:237)"""
    j = np.float32(1.0 * shared / s)
    if j == 0:
        md = np.float32(1.0)
    elif j == 1:
        md = np.float32(0.0)
    else:
        md = np.float32((-1.0 / k) * math.log(2.0 * float(j) / float(np.float32(1) + j)))
    return text6(float(np.float32(100) * (np.float32(1) - md))) / 100.0


def success_p(best_identity: float, read_len: int, k: int) -> float:
    """mapWrap.h:261-266, :335-339 in float64 (mapq_success_p)"""
    maxid = math.exp(-(1 - best_identity))
    nk = read_len - k + 1
    surv = math.pow(maxid, float(k))
    es = float(math.floor(surv * nk + 0.5))                       # C's round() of a non-negative value
    eu = nk + (nk - es)
    return es / eu


def pmf_exact(n: int, p: float, k: int):
    """the binomial mass of k successes in n trials with the DOUBLE p, as an mpf"""
    if k < 0 or k > n:
        return mpmath.mpf(0)
    P = mpmath.mpf(p)
    return mpmath.binomial(n, k) * P ** k * (1 - P) ** (n - k)


def pmf_float64(n: int, p: float, k: int) -> float:
    """dev_binom_pmf restated in float64 (boost pdf(binomial), mapWrap.h:340)"""
    if k < 0 or k > n:
        return 0.0
    if p == 0:
        return 1.0 if k == 0 else 0.0
    if p == 1:
        return 1.0 if k == n else 0.0
    if n == 0:
        return 1.0
    if k == 0:
        return math.pow(1 - p, float(n))
    if k == n:
        return math.pow(p, float(k))
    x = math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0) + k * math.log(p) + (n - k) * math.log1p(-p)
    return math.exp(x) if x > -745.2 else 0.0


def pmf_scale(n: int, p: float, k: int) -> float:
    """S: the error of dev_binom_pmf is at most about S ulps (2^-52) relative.
    Inside (0 < k < n, 0 < p < 1) the mass is exp of a sum of five terms; each term carries a relative error of an ulp or so (lgamma, log, log1p,
    the products) and the additions as much of their partial sums, so the exponent is off by about (sum of |terms|) ulps absolutely, which is the
    relative error of its exp.  At k == 0 and k == n the mass is pow(base, n): the base 1 - p carries half an ulp and is raised to the n, pow
    adds an ulp or so of its own: n + 1.  Where the code returns a constant (p == 0, p == 1, n == 0, k outside), S is 0: exact."""
    if k < 0 or k > n or p == 0 or p == 1 or n == 0:
        return 0.0
    if k == 0 or k == n:
        return float(n + 1)
    return (math.lgamma(n + 1.0) + math.lgamma(k + 1.0) + math.lgamma(n - k + 1.0) + abs(k * math.log(p)) + abs((n - k) * math.log1p(-p)))


# err / (S * 2^-52) of the HOST build of dev_binom_pmf over the grid of test_post_core.py::test_binom_pmf_against_exact_mass, masses above 1e-290:
# measured worst 0.8133 (n = 32 768, p = 0.0207, k = 326, a mass of 3.2e-84); the bound is twice that.
PMF_C_HOST = 1.6266
# The device's lgamma, log1p, exp and pow carry looser ulp bounds than glibc's: four times the host's constant for a mass, and twice that for a
# normalised quality (numerator and sum each err: test_gpu_post_edges.py::exact_qualities adds the S of the record and the weighted S of the sum).
# Measured on an MI355X over test_k8_qualities_against_exact_masses, 1 826 qualities above 1e-290: worst error 0.0415 of that bound, which is
# 0.27 in units of (S + S_sum) * 2^-52 (the float64 restatement on the host: 0.0361 of the bound).
PMF_C_DEVICE = 4 * PMF_C_HOST


def stop_now(it: int, ll: float, ll_prev: float) -> bool:
    """fEM.h:624-639 (em_stop_now)"""
    return it > 0 and (ll - ll_prev) <= 1 and (1 - ll / ll_prev) < 0.0001


def em_reference(read_off, taxon, mapq, inv_nloc, n_taxa, f0, max_iter=1000, w=None):
    """float64 EM with the reference's order of products (f * 1/nLoc * mapq, fEM.h:353) and exact sums over the mappings of a read, the
    posteriors of a taxon and the reads' logs.  Returns (f, log-likelihoods, margins): margins[i] = how far, relatively, the two stop quantities
    of iteration i stand off their thresholds (gain vs 1, 1 - ll / ll_prev vs 1e-4).  It ends with the stop rule or after max_iter iterations.
    w: an integer weight per read (the bootstrap's weighted EM, mm_boot.hip): posteriors are w[r] * l / S[r], the log-likelihood sums
    w[r] * log S[r], a read with w == 0 adds nothing.  A weighted sample without a mapped read of w > 0 has no estimate: (zeros, no
    log-likelihood, no margins) — what boot_expected turns into the library's empty replicate."""
    read_off = np.asarray(read_off, dtype=np.int64); taxon = np.asarray(taxon, dtype=np.int64)
    inv = np.asarray(inv_nloc, dtype=np.float64); q = np.asarray(mapq, dtype=np.float64)
    f = np.asarray(f0, dtype=np.float64).copy()
    sizes = np.diff(read_off)
    wr = np.ones(len(sizes)) if w is None else np.asarray(w, dtype=np.float64)
    assert wr.shape == sizes.shape and np.all(wr >= 0) and np.all(wr == np.floor(wr))
    full = np.nonzero((sizes > 0) & (wr > 0))[0]
    if len(full) == 0:
        return np.zeros(n_taxa), np.zeros(0), []
    by_taxon = [np.nonzero(taxon == t)[0] for t in range(n_taxa)] if len(taxon) < 200_000 else None
    if by_taxon is None:
        order = np.argsort(taxon, kind="stable"); cut = np.searchsorted(taxon[order], np.arange(n_taxa + 1))
        by_taxon = [order[cut[t]:cut[t + 1]] for t in range(n_taxa)]
    w_entry = np.repeat(wr, sizes)
    lls, margins = [], []
    ll_prev = 0.0
    for it in range(max_iter):
        l = f[taxon] * inv * q
        sums = np.ones(len(sizes))                                  # (reads that are not in the sample: their posteriors are w * l / 1 = 0)
        for r in full:
            sums[r] = math.fsum(l[read_off[r]:read_off[r + 1]])
        post = w_entry * l / np.repeat(sums, sizes)
        ll = math.fsum(wr[r] * math.log(sums[r]) for r in full)
        tot = np.array([math.fsum(post[ix]) for ix in by_taxon])
        f = tot / math.fsum(tot)
        lls.append(ll)
        if it > 0:
            margins.append((abs((ll - ll_prev) - 1), abs((1 - ll / ll_prev) - 0.0001) / 0.0001))
        stop = stop_now(it, ll, ll_prev)
        ll_prev = ll
        if stop:
            break
    return f, np.array(lls), margins


def boot_weights(read_off, seed=None, rep=None, row=None):
    """the weight of every read in one replicate of the bootstrap: weights_np(seed, rep, i) — or row[i], one row of caller weights — for the
    i-th read WITH a mapping, in read order; 0 for a read without one (it is not resampled)"""
    from test_boot_core import weights_np
    mapped = np.diff(np.asarray(read_off, dtype=np.int64)) > 0
    n_mapped = int(np.count_nonzero(mapped))
    w = np.zeros(len(mapped), dtype=np.int64)
    if row is None:
        w[mapped] = weights_np(np.uint64(seed), np.uint64(rep), np.arange(n_mapped, dtype=np.uint64))
    else:
        row = np.asarray(row)
        assert row.shape == (n_mapped,)
        w[mapped] = row
    return w


def boot_expected(read_off, taxon, mapq, inv_nloc, n_taxa, f_start, w, max_iter=10_000):
    """what mm_em_bootstrap reports for one replicate of weights w: (f, ll, n_iter, stopped, margins).  An empty weighted sample is
    f = 0, ll = 0, no iteration, stopped."""
    f, lls, margins = em_reference(read_off, taxon, mapq, inv_nloc, n_taxa, f_start, max_iter=max_iter, w=w)
    if len(lls) == 0:
        return f, 0.0, 0, True, margins
    stopped = stop_now(len(lls) - 1, lls[-1], lls[-2] if len(lls) > 1 else 0.0)
    return f, float(lls[-1]), len(lls), bool(stopped), margins


def posteriors_reference(read_off, taxon, mapq, inv_nloc, f):
    """the E step alone in float64 with exact read sums: (posteriors, log-likelihood); a read without mappings adds nothing"""
    read_off = np.asarray(read_off, dtype=np.int64)
    l = np.asarray(f, dtype=np.float64)[np.asarray(taxon, dtype=np.int64)] * np.asarray(inv_nloc, dtype=np.float64) * np.asarray(mapq, dtype=np.float64)
    sizes = np.diff(read_off)
    sums = np.array([math.fsum(l[read_off[r]:read_off[r + 1]]) for r in range(len(sizes))])
    with np.errstate(invalid="ignore", divide="ignore"):
        post = l / np.repeat(sums, sizes)
    ll = math.fsum(math.log(s) for s, n in zip(sums, sizes) if n)
    return post, ll
