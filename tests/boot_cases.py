"""The problems, weights and (problem, replicate) pairs on which tests/test_gpu_boot_edges.py holds the bootstrap EM (mm_boot.hip) to the exact
weighted reference (post_ref.em_reference), and that reference's answer for each pair.  tests/test_boot_cases.py checks on the CPU that the
cases are what the GPU tests take them for (reads whose index among the mapped reads is not their index, empty replicates, replicates of one
tile that stop in different iterations, stop margins).  Nothing here touches the device or the library."""
import functools

import numpy as np

import post_ref
from test_gpu_post_edges import LOOP_PROBLEMS, random_entries

SEED = 7                                                           # of the generated weights
MAX_ITER = 10_000
ROWS_PRESENT = (3, 15, 16, 17)                                     # present taxa against P3b's 16 rows of lanes
ROWS_WORKGROUPS = (1, 15, 16, 17)                                  # workgroups of P1b (their partial log-likelihoods) against the same rows


def problem_three_reads():
    """three mapped reads with an unmapped one before, between and after; taxa 1 and 3 of five have entries"""
    rng = np.random.default_rng(921)
    off, _, mapq, inv = random_entries(rng, [0, 2, 0, 3, 0, 2, 0], 5)
    return off, np.array([1, 3, 3, 1, 3, 1, 3], dtype=np.int32), mapq, inv, 5


def problem_one_read():
    rng = np.random.default_rng(922)
    off, _, mapq, inv = random_entries(rng, [0, 3, 0], 4)
    return off, np.array([2, 0, 2], dtype=np.int32), mapq, inv, 4


def problem_no_mapping():
    return np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), 3


def problem_fewer_reads_than_rows(n_present, n_taxa=20):
    """40 reads of 0 .. 4 mappings (fewer reads than the 256 workgroups of the default grid) on n_present taxa of n_taxa"""
    rng = np.random.default_rng(930 + n_present)
    taxa = np.sort(rng.choice(n_taxa, n_present, replace=False))
    sizes = rng.integers(0, 5, 40)
    sizes[[0, 39]] = 0
    off, taxon, mapq, inv = random_entries(rng, sizes, n_taxa, taxa)
    assert len(taxon) >= n_present
    taxon[:n_present] = taxa                                        # every present taxon at least once
    return off, taxon, mapq, inv, n_taxa


def problem_workgroups(n_reads):
    """n_reads reads of 0 .. 4 mappings on six taxa: the default grid has one workgroup per read, so P3b's 16 rows add n_reads partial
    log-likelihoods"""
    rng = np.random.default_rng(960 + n_reads)
    sizes = rng.integers(0, 5, n_reads)
    sizes[0] = 3
    return random_entries(rng, sizes, 6) + (6,)


def problem_slow():
    """Two taxa that 30 reads cannot tell apart well (qualities 1 and 0.9, one location each) and two reads of their own each: the EM creeps,
    and the replicates stop after 16 to 54 iterations — on either side of every max_iter at boot_run's 24 | 8 | 8 groups"""
    sizes = [0] + [1] * 2 + [2] * 30 + [0] + [1] * 2
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    taxon = np.array([0] * 2 + [0, 2] * 30 + [2] * 2, dtype=np.int32)
    mapq = np.array([1.0] * 2 + [1.0, 0.9] * 30 + [1.0] * 2)
    return off, taxon, mapq, np.ones(len(taxon)), 3


PROBLEMS = dict(LOOP_PROBLEMS)
PROBLEMS.update({"three_reads": problem_three_reads, "one_read": problem_one_read, "no_mapping": problem_no_mapping, "slow": problem_slow})
PROBLEMS.update({f"fewer_reads_than_rows_{n}": functools.partial(problem_fewer_reads_than_rows, n) for n in ROWS_PRESENT})
PROBLEMS.update({f"workgroups_{n}": functools.partial(problem_workgroups, n) for n in ROWS_WORKGROUPS})


@functools.lru_cache(maxsize=None)
def problem(name):
    p = PROBLEMS[name]()
    for a in p[:4]:
        a.setflags(write=False)
    return p


def f_start(name):
    """every replicate starts from the uniform frequencies (further from its estimate than the point estimate is: more iterations)"""
    T = problem(name)[4]
    return np.full(T, 1.0 / T)


def mapped_reads(name):
    return int(np.count_nonzero(np.diff(problem(name)[0])))


def generated_matrix(name, rep0, n_rep, seed=SEED):
    """[n_rep][n_mapped]: the generated weights of replicates rep0 .. rep0 + n_rep - 1"""
    from test_boot_core import weights_np
    n = mapped_reads(name)
    return weights_np(np.uint64(seed), np.arange(rep0, rep0 + n_rep, dtype=np.uint64)[:, None], np.arange(n, dtype=np.uint64)[None, :]).reshape(n_rep, n)


def empty_replicates(name, n_rep, rep0=0, seed=SEED):
    return [rep0 + r for r, row in enumerate(generated_matrix(name, rep0, n_rep, seed)) if not row.any()]


def caller_rows(name):
    """caller weights for `name`: three rows drawn from {0, 1, 2, 255} and a row of ones (the second)"""
    rng = np.random.default_rng(951)
    w = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=(4, mapped_reads(name)))
    w[1] = 1
    return w


def zero_row_between_ones(name):
    w = np.ones((3, mapped_reads(name)), dtype=np.uint8)
    w[1] = 0
    return w


@functools.lru_cache(maxsize=None)
def expected(name, rep=None, caller=None, row=None, max_iter=MAX_ITER):
    """the reference's (f, ll, n_iter, stopped, margins) of replicate `rep` of the generated weights on problem `name`, or of row `row` of the
    caller weights `caller` ("rows": caller_rows, "zero_row": zero_row_between_ones)"""
    off, taxon, mapq, inv, T = problem(name)
    if caller is None:
        w = post_ref.boot_weights(off, SEED, rep)
    else:
        w = post_ref.boot_weights(off, row={"rows": caller_rows, "zero_row": zero_row_between_ones}[caller](name)[row])
    return post_ref.boot_expected(off, taxon, mapq, inv, T, f_start(name), w, max_iter=max_iter)


def iterations(name, reps):
    return [expected(name, r)[2] for r in reps]


# ----------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests compare with the reference
# ----------------------------------------------------------------------------------------------------------------------------------
# The stop rule must not flip on rounding.  The smallest margin of the reference's last two iterations (|gain - 1| and |1 - ll / ll_prev - 1e-4| / 1e-4,
# whichever is smaller) over the compared replicates, and their iteration counts, as measured when the seeds (7 for the weights, those of the
# problems) were chosen — test_boot_cases.py asserts at least 1e-6 for every pair:
#   generated weights, replicates 0, 1, 63, 64 (and 0 .. 128 of the tile problem's earliest and latest stopper):
#     mappings_per_read 1.8e-3 (8 .. 12 iterations), skewed_reads 0.85 (4), entries_per_taxon 0.017 (5, 6), present_1_of_300 1 (3),
#     present_255 / 256 / 257_of_300 0.025 / 3.4e-3 / 0.04 (5, 6), one_taxon 1 (2), fewer_reads_than_rows_3 / 15 / 16 / 17 0.096 / 0.16 / 0.12 /
#     0.081 (4 .. 6), workgroups_1 / 15 / 16 / 17 0.32 / 0.088 / 0.22 / 0.046 (8; 4, 5; 4, 5; 3 .. 6), one_read 0.39 (3); replicates 1 and 63 of
#     one_read and of workgroups_1 are empty
#   caller weights on mappings_per_read 0.016 (9 .. 12); slow, replicates 0 .. 3, at every cap 0.03 (17, 54, 16 and 26 iterations uncapped);
#   three_reads, replicates 0 .. 128, 0.32 (3, 4; six empty), with the row of zeros 0.98
GENERATED = list(LOOP_PROBLEMS) + [f"fewer_reads_than_rows_{n}" for n in ROWS_PRESENT] + [f"workgroups_{n}" for n in ROWS_WORKGROUPS] + ["one_read"]
GENERATED_B = 65
GENERATED_REPS = (0, 1, 63, 64)
# further replicates: of the one mapped read of one_read and of workgroups_1, 1 and 63 are empty, 0 and 64 draw it once, 2 twice
MARKED = {"one_read": (2,), "workgroups_1": (2,)}

TILE = "mappings_per_read"                                         # the tile problem: replicates 0 .. 64 stop in 8 to 13 iterations
TILE_B = (63, 64, 65, 128, 129)


def tile_reps():
    """replicates 0, 63, 64 and the earliest and the latest stopper of 0 .. 128"""
    it = iterations(TILE, range(129))
    return sorted({0, 63, 64, int(np.argmin(it)), int(np.argmax(it))})


CAPS = (1, 23, 24, 25, 32, 33)
CAP_B = 4
BIG_REP0, BIG_N = 2**31 - 10, 10
BIG = "fewer_reads_than_rows_17"
BIG_REPS = (BIG_REP0, 2**31 - 1)
EMPTY, EMPTY_B = "three_reads", 129


def compared():
    """every (problem, replicate, caller weights, row, max_iter) that a GPU test compares with the reference"""
    out = [(n, r, None, None, MAX_ITER) for n in GENERATED for r in GENERATED_REPS + tuple(MARKED.get(n, ()))]
    out += [("mappings_per_read", None, "rows", k, MAX_ITER) for k in range(4)]
    out += [(TILE, r, None, None, MAX_ITER) for r in tile_reps()]
    out += [("slow", r, None, None, cap) for cap in CAPS for r in range(CAP_B)]
    out += [(BIG, r, None, None, MAX_ITER) for r in BIG_REPS]
    out += [(EMPTY, r, None, None, MAX_ITER) for r in range(EMPTY_B)]
    out += [(EMPTY, None, "zero_row", k, MAX_ITER) for k in range(3)]
    return list(dict.fromkeys(out))
