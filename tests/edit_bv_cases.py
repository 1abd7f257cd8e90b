"""Problems for the bit-vector edit-distance tests beyond tests/edit_cases.py: the ladder of read lengths at which a lane of the pipeline gets
another block (metamaps_amd/csrc/mm_edit_bv_core.hpp: blocks of W = 32 rows, 64 lanes) and the windows shorter than the pipeline.  Each problem is
(read, strand, window, max_dist) as in edit_cases."""
import edit_cases
import edit_ref

W = 32
LADDER = (0, 1, W - 1, W, W + 1, 64 * W - 1, 64 * W, 64 * W + 1, 128 * W + 1)      # the last three: a lane gets its second and its third block


def exact_read(rng, src, m, rate, dirt):
    """a read of exactly m bases made from src with errors, N / IUPAC and lower case sprinkled"""
    r = edit_cases.mutate(rng, src, rate)[:m]
    r += edit_cases.dna(rng, m - len(r))
    return edit_cases.sprinkle(rng, r, dirt, b"NnMS") if dirt else r


def ladder_problems(rng, ladder=LADDER):
    """every m of the ladder on both strands at 10 % errors, each with n < 64, n = m and n = m + 2 pad"""
    out = []
    for m in ladder:
        pad = edit_ref.pad(m)
        for strand in (1, -1):
            win = edit_cases.sprinkle(rng, edit_cases.dna(rng, m + 2 * pad), 0.02, b"NRYK")
            read = edit_cases.stored(exact_read(rng, win[pad:pad + m], m, 0.1, 0.02), strand)
            out.append((read, strand, win[pad:pad + min(m, 40 + m % 23)], None))       # n < 64
            out.append((read, strand, win[pad:pad + m], None))                         # n = m
            out.append((read, strand, win, edit_ref.cap(m, 70.0)))                     # n = m + 2 pad, by the cap rule
    return out


def short_window_problems(rng, m=64 * W + 52):
    """a read of more than 64 blocks against windows shorter than the pipeline is deep"""
    win = edit_cases.dna(rng, 80)
    read = exact_read(rng, win + edit_cases.dna(rng, m), m, 0.05, 0.0)
    return [(edit_cases.stored(read, s), s, win[:n], None) for n in (0, 1, 63, 64, 65) for s in (1, -1)]
