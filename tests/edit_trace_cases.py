"""Problems for the alignment (CIGAR) tests that the random ones do not reach (metamaps_amd/csrc/mm_edit_trace_core.hpp: blocks of 32 rows, strips
of 64 columns, lane 0 of a read of more than 2048 bases owns the first 64 rows of the reversed read, which are the read's last 64 bases).  Each
problem is (read, strand, window, max_dist) as in edit_cases."""
import edit_cases
import edit_cigar_ref

INS, DEL = 100, 150


def _insertion(rng, m_left, m_right):
    """INS bases that match nothing between two stretches of the window: the walk climbs INS rows in one column"""
    win = edit_cases.dna(rng, 30 + m_left + m_right + 30)
    return win[30:30 + m_left] + b"N" * INS + win[30 + m_left:30 + m_left + m_right], 1, win, None


def _deletion(rng, m_left, m_right, gone=DEL):
    """`gone` window bases that the read skips: the walk crosses that many columns in one row.  They match nothing (the walk takes = wherever two
    bases match, which would cut the run into pieces).  The read's ends are global and the window's are free, so the deletion is the best alignment
    only while it costs less than leaving the shorter flank unaligned: gone < min(m_left, m_right)"""
    win = edit_cases.dna(rng, 30 + m_left + gone + m_right + 30)
    win = win[:30 + m_left] + b"N" * gone + win[30 + m_left + gone:]
    return win[30:30 + m_left] + win[30 + m_left + gone:30 + m_left + gone + m_right], 1, win, None


SHORT = 60


def built_problems(rng):
    out = [_insertion(rng, 150, 150), _deletion(rng, 400, 400)]
    # m = 2100: B = 2, lane l owns rows [64 l, 64 l + 64) of the reversed read, which are the read's last bases.  The insertion ends 20 bases before
    # the read's end: it climbs from lane 1 into lane 0.  A deletion of DEL bases cannot lie 64 bases before the read's end (see _deletion): it lies
    # in row 1024, the first of lane 16, and one of SHORT bases lies in row 64, the first of lane 1.
    out += [_insertion(rng, 2100 - INS - 20, 20), _deletion(rng, 2100 - 1025, 1025), _deletion(rng, 2100 - 65, 65, SHORT)]
    win = edit_cases.dna(rng, 500)
    out.append((win[100:400], 1, win, None))                                          # an exact match: one run
    out.append((edit_cases.stored(win[100:400], -1), -1, win, 0))
    return out


def longest(runs, op):
    return max([int(w) >> 4 for w in runs if (int(w) & 15) == op], default=0)


def check_built(problems, answers):
    """the cases are what they are built to be (asked of the reference's answers)"""
    assert [longest(a[3], edit_cigar_ref.OP_I) for a in answers[:5]] == [INS, 0, INS, 0, 0]
    assert [longest(a[3], edit_cigar_ref.OP_D) for a in answers[:5]] == [0, DEL, 0, DEL, SHORT]
    assert [len(p[0]) for p in problems[2:5]] == [2100, 2100, 2100]
    assert [edit_cigar_ref.cigar(a[3]) for a in answers[5:]] == ["300=", "300="] and answers[5][:3] == (0, 100, 400)
