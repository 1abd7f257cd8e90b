"""The plain restatement of mapDirectly --depth / mm_depth_profile (the definition: metamaps_amd/csrc/mm_depth_core.hpp): one numpy array of depths per contig,
filled interval by interval, and everything read off it position by position.  No breakpoints, no sorting of interval ends, no prefix sums: it shares nothing
with the event form the device runs.  Also the three texts of PREFIX.depth.bedgraph, .depth.windows and .depth.contigs."""
import math

import numpy as np

STATS = ("alignments", "covered", "sumDepth", "medianDepth", "maxDepth")
MAX_LEN = (1 << 29) - 1
MAX_THRESHOLDS = 8


def refused(lens, iv, window, thresholds):
    """why the call is refused, or None"""
    if any(not 1 <= n <= MAX_LEN for n in lens):
        return "length"
    if window < 1:
        return "window"
    if len(thresholds) > MAX_THRESHOLDS or any(t < 1 for t in thresholds) or any(a >= b for a, b in zip(thresholds, thresholds[1:])):
        return "thresholds"
    for k, (c, a, b) in enumerate(iv):
        if not (0 <= c < len(lens) and 0 <= a <= b < lens[c]):
            return f"interval {k}"
    return None


def depths(lens, iv):
    """{contig: its depths} for the contigs with an interval"""
    d = {}
    for c, a, b in iv:
        if c not in d:
            d[c] = np.zeros(lens[c], dtype=np.int64)
        d[c][a:b + 1] += 1
    return d


def profile(lens, iv, window=1000, thresholds=(1, 5, 10, 30)):
    """dict(runs=[(contig, start, end, depth)], contig=[...], win_off=[...], stats=[[STATS..., ge...]], win_sum=[...], win_covered=[...])"""
    assert refused(lens, iv, window, thresholds) is None
    d = depths(lens, iv)
    runs, contig, win_off, stats, win_sum, win_covered = [], [], [0], [], [], []
    for c in sorted(d):
        x = d[c]
        n = len(x)
        p = 0
        while p < n:                                                # the maximal runs of equal depth, position by position
            q = p
            while q < n and x[q] == x[p]:
                q += 1
            if x[p] > 0:
                runs.append((c, p, q, int(x[p])))
            p = q
        contig.append(c)
        stats.append([sum(1 for cc, _, _ in iv if cc == c), int((x > 0).sum()), int(x.sum()), int(np.sort(x)[(n - 1) // 2]), int(x.max())] + [int((x >= t).sum()) for t in thresholds])
        for a in range(0, n, window):
            win_sum.append(int(x[a:a + window].sum()))
            win_covered.append(int((x[a:a + window] > 0).sum()))
        win_off.append(len(win_sum))
    return dict(runs=runs, contig=contig, win_off=win_off, stats=stats, win_sum=win_sum, win_covered=win_covered)


def bedgraph_text(res, cname):
    return "".join(f"{cname[c]}\t{a}\t{b}\t{d}\n" for c, a, b, d in res["runs"])


def windows_text(res, cname, lens, window):
    out = []
    for j, c in enumerate(res["contig"]):
        for k in range(res["win_off"][j], res["win_off"][j + 1]):
            a = (k - res["win_off"][j]) * window
            b = min(a + window, lens[c])
            out.append(f"{cname[c]}\t{a}\t{b}\t{res['win_sum'][k]}\t{res['win_covered'][k]}\t{res['win_sum'][k] / (b - a):.3f}\n")
    return "".join(out)


def contigs_header(thresholds):
    return "#contigID\tlength\talignments\tcovered\tsumDepth\tmeanDepth\tmedianDepth\tmaxDepth\tbreadth\texpectedBreadth" + "".join(f"\tge{t}" for t in thresholds) + "\n"


def contigs_text(res, cname, lens, thresholds):
    out = [contigs_header(thresholds)]
    for c, s in zip(res["contig"], res["stats"]):
        n = lens[c]
        al, cov, total, med, mx = s[:5]
        out.append(f"{cname[c]}\t{n}\t{al}\t{cov}\t{total}\t{total / n:.3f}\t{med}\t{mx}\t{cov / n:.6f}\t{1 - math.exp(-total / n):.6f}" + "".join(f"\t{g}" for g in s[5:]) + "\n")
    return "".join(out)
