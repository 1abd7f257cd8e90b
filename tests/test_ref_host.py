"""The two readers of this repository — the CLI's (metamaps_amd/csrc/host/seq_reader.hpp: sequential, block-parallel over a
memory-mapped file, zlib) and the oracle's (oracle/orc_io.hpp) — against the REFERENCE'S OWN reader: oracle/_ref/ref_host is
/root/reference/src/common/kseq.h compiled where it lies (oracle/Makefile, target `ref`; no Boost needed).  Same for the
reference's meta/util.h split() and overlap() against the host's and the oracle's.  This turns the FASTA/FASTQ layer under
every sequence the path ever sees (winSketch.hpp:245-252, computeMap.hpp:123-134, mapWrap.h:107-114) from "restated" into
"pinned by reference code run here".

What the reference's code answered on every input below is pinned in tests/golden/ref_golden.json (sha256 digests, written by
tests/golden/make_ref_golden.py from oracle/_ref/ref_host), so that these tests need nothing outside the repository.  Where
oracle/_ref/ is built (__graft_entry__.build() builds it wherever the reference tree exists) the live reference is run as well and
must still give the pinned answers.

CPU only."""
import ctypes as C
import gzip
import hashlib
import json
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(ROOT, "oracle", "_ref", "ref_host")
GOLDEN = os.path.join(HERE, "golden", "ref_golden.json")


class Ref:
    """the reference's answers: the pinned digests, and the live oracle/_ref/ref_host where it is built (None elsewhere)"""
    def __init__(self, exe):
        self.exe = exe
        self.golden = json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def ref():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, timeout=600)   # (a no-op without the reference tree)
    return Ref(REF if os.path.exists(REF) else None)


def digest(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()[:24]


def kseq_digest(lines, code) -> str:
    """one digest over the records of a read loop and the code that ended it (the output format of `ref_host kseq`)"""
    return digest(("".join(l + "\n" for l in lines) + "END %d\n" % code).encode("latin-1"))


@pytest.fixture(scope="module")
def host_reader(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("rh") / "seq")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", e, os.path.join(HERE, "test_seq_reader.cpp"), "-lz"], check=True, timeout=300)
    return e


@pytest.fixture(scope="module")
def host_util(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("rh") / "util")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", e, os.path.join(HERE, "test_host_util.cpp"), "-lz"], check=True, timeout=300)
    return e


def _kseq(exe, path):
    """records of the real kseq_read loop (or None where the reference itself crashes, e.g. an empty first record: kseq.h:189
    writes through a buffer it never allocated)"""
    r = subprocess.run([exe, "kseq", path], capture_output=True, timeout=120)
    if r.returncode != 0:
        return None
    lines = r.stdout.decode("latin-1").splitlines()
    assert lines and lines[-1].startswith("END ")
    return lines[:-1], int(lines[-1].split()[1])


def _oracle_reader(oracle_lib, path):
    buf = C.create_string_buffer(1 << 22)
    oracle_lib.L.orc_read_dump.restype = C.c_long
    oracle_lib.L.orc_read_dump.argtypes = [C.c_char_p, C.c_char_p, C.c_long]
    n = oracle_lib.L.orc_read_dump(path.encode(), buf, len(buf))
    assert n >= 0
    lines = buf.raw[:n].decode("latin-1").splitlines()
    return lines[:-1], int(lines[-1].split()[1])


def _host_reader(exe, path):
    """sequential records, and whether every block size of the block parser reproduced them"""
    seq = subprocess.run([exe, path, "dump"], capture_output=True, timeout=120).stdout.decode("latin-1").splitlines()
    blocks_ok = None
    if os.path.getsize(path) >= 4 and not path.endswith(".gz"):
        r = subprocess.run([exe, path], capture_output=True, timeout=120)
        blocks_ok = r.returncode == 0 and b"ok" in r.stdout
    return seq, blocks_ok


def _check(ref, oracle_lib, exe, path, key):
    """the oracle's and the host's readers against what the reference's reader gave on this input (pinned under `key`);
    False where the reference crashes on it"""
    pin = ref.golden["kseq"][key]
    if ref.exe is not None:
        k = _kseq(ref.exe, path)
        assert (k and [kseq_digest(*k), len(k[0])]) == (pin or None), (key, "the live reference no longer gives the pinned answer")
    if pin is None:
        return False
    want, n_want = pin
    got_o, code_o = _oracle_reader(oracle_lib, path)
    assert kseq_digest(got_o, code_o) == want, (key, "oracle reader", len(got_o), n_want)
    got_h, blocks_ok = _host_reader(exe, path)
    assert got_h == got_o, (key, "host reader", len(got_h), n_want)
    assert blocks_ok in (None, True), (key, "block parser differs from the sequential parse")
    return True


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


# name -> file content; every layout starts with a record that has bases (kseq.h:189 dereferences an unallocated buffer otherwise)
def _layouts():
    rng = random.Random(77)
    s = [_seq(rng, n) for n in (50, 4000, 1, 77, 5000, 300, 12, 4096, 4095, 9000)]
    q = ["I" * len(x) for x in s]
    fq = lambda i, name=None: f"@{name or 'r%d' % i} c{i}\n{s[i]}\n+\n{q[i]}\n"
    L = {}
    L["plain"] = "".join(fq(i) for i in range(10))
    L["no_final_newline"] = L["plain"][:-1]
    L["crlf"] = L["plain"].replace("\n", "\r\n")
    L["fasta_wrapped"] = "".join(f">c{i} d\n" + "\n".join(s[i][j:j + 60] for j in range(0, len(s[i]), 60)) + "\n" for i in range(10))
    L["fasta_lowercase_N_iupac"] = ">a\n" + _seq(rng, 500, "acgtnNRYKM") + "\n>b x\n" + _seq(rng, 70, "acgt") + "\n"
    L["quality_longer_than_sequence"] = fq(0) + f"@long\n{s[1]}\n+\n{q[1]}IIIII\n" + fq(2) + fq(3)
    L["quality_longer_with_header_chars"] = fq(0) + f"@long\n{s[3]}\n+\n{q[3]}@>@I\n" + fq(2) + fq(4)
    L["quality_shorter_than_sequence"] = fq(0) + f"@short\n{s[1]}\n+\n{q[1][:-7]}\n" + fq(2) + fq(3)
    L["quality_truncated_at_eof"] = fq(0) + fq(1) + f"@t\n{s[2]}{s[3]}\n+\n{q[3][:5]}"
    L["no_newline_before_next_record"] = fq(0)[:-1] + fq(1) + fq(2)[:-1] + fq(3)
    L["plus_inside_fasta_line"] = f">p1\n{s[0]}+{s[2]}\n{s[3]}\n>p2\n{s[5]}\n"
    L["at_and_gt_inside_sequence_lines"] = f"@x\n{s[0]}@{s[3]}\n+\n" + "I" * (len(s[0])) + "\n" + fq(5) + f">y\n{s[6]}>{s[6]}\n" + fq(7)
    L["wrapped_fastq"] = fq(0) + f"@w\n{s[4][:2000]}\n{s[4][2000:]}\n+w\n{q[4][:100]}\n{q[4][100:]}\n" + fq(5)
    L["quality_with_header_chars"] = fq(0) + f"@n1\n{s[3]}\n+\n" + _seq(rng, len(s[3]), "@>+I!~5") + "\n" + fq(6) + f"@n2\n{s[5]}\n+\n@" + "I" * (len(s[5]) - 1) + "\n" + fq(2)
    L["blank_lines_tabs_spaces"] = f"\n\n@r a\tb\n{s[0][:20]} {s[0][20:]}\t\n\n+\n{q[0]}\n\n\n" + f"@t\tx y\n{s[3]}\n+\n{q[3]}\n" + f">f\tz\n{s[6]}\n\n{s[6]}\n"
    L["garbage_before_first_record"] = "garbage line\nmore\n" + fq(0) + fq(1)
    L["empty_name"] = f"@\n{s[0]}\n+\n{q[0]}\n> \n{s[3]}\n" + fq(5)
    L["empty_sequence_later"] = fq(0) + "@e\n\n+\n\n" + fq(3) + ">ef\n>g\n" + s[6] + "\n"
    L["header_only_at_eof"] = fq(0) + "@last"
    L["header_char_at_eof"] = fq(0) + "@"
    L["plus_line_at_eof"] = fq(0) + f"@p\n{s[3]}\n+"
    L["high_bytes"] = fq(0) + f"@h\n{s[3][:10]}\x80\xc3{s[3][10:]}\n+\n{q[3]}\n" + fq(2)
    L["mixed_fasta_fastq"] = fq(0) + f">m\n{s[5]}\n" + fq(6) + f">n\n{s[7]}\n"
    L["empty_file"] = ""
    L["no_record"] = "just text\nno header\n"
    L["buffer_boundary_name"] = "@" + "n" * 4090 + " c\n" + s[0] + "\n+\n" + q[0] + "\n" + fq(8) + fq(9)
    return L


LAYOUTS = _layouts()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_readers_equal_real_kseq(ref, oracle_lib, host_reader, tmp_path, layout):
    p = str(tmp_path / "in.fq")
    with open(p, "wb") as f:
        f.write(LAYOUTS[layout].encode("latin-1"))
    assert _check(ref, oracle_lib, host_reader, p, layout), "the reference's reader crashed on a curated layout"
    with open(p, "rb") as f, gzip.open(p + ".gz", "wb") as g:    # the same bytes through zlib (winSketch.hpp:245-248 opens everything with gzopen)
        g.write(f.read())
    assert _check(ref, oracle_lib, host_reader, p + ".gz", layout + ".gz")
    if layout == "no_newline_before_next_record":               # the quirk is observable: kseq.h:200 eats the '@' that follows the qualities
        assert [l.split()[0] for l in _oracle_reader(oracle_lib, p)[0]] == ["r0", "r2"]   # (the oracle's records are the reference's: _check)


def soup(seed):
    """the file of byte soup number `seed`"""
    rng = random.Random(seed)
    kind = seed % 4
    if kind == 0:     # pure soup
        alpha = "@>+\n\n\r \tACGTacgtnN!~I5" + ("\x80" if seed % 8 == 0 else "")
        body = "".join(rng.choice(alpha) for _ in range(rng.choice([30, 300, 5000, 20000])))
    else:             # records with random damage
        parts = []
        for i in range(rng.randrange(1, 25)):
            n = rng.choice([1, 5, 60, 200, 1500, 4096, 6000])
            sq = _seq(rng, n, "ACGTacgtN")
            ql = n + rng.choice([0, 0, 0, 0, 1, -1, 5, -5]) if kind == 3 else n
            qu = _seq(rng, max(ql, 0), "I5?~!@>+" if kind >= 2 else "I5?~!")
            if rng.random() < 0.3:
                parts.append(f">f{i} c\n" + "\n".join(sq[j:j + 70] for j in range(0, n, 70)) + "\n")
            else:
                nl = "" if (kind == 3 and rng.random() < 0.2) else "\n"
                wrap = rng.random() < 0.2 and n > 10
                sl = sq[:n // 2] + "\n" + sq[n // 2:] if wrap else sq
                parts.append(f"@q{i}{rng.choice(['', ' c', chr(9) + 'c'])}\n{sl}\n+{rng.choice(['', 'x'])}\n{qu}{nl}")
        body = "".join(parts)
        if kind == 3 and rng.random() < 0.5:
            body = body[:rng.randrange(len(body) // 2, len(body))]
    return "@first\nACGT\n+\nIIII\n" + body


SOUP_SEEDS = range(500)


def test_readers_equal_real_kseq_on_byte_soup(ref, oracle_lib, host_reader, tmp_path):
    """random files over an alphabet of everything kseq treats specially: 500 seeds, 30 bytes to 20 kb (kseq's buffer is 4096 bytes)"""
    crashed = 0
    for seed in SOUP_SEEDS:
        body = soup(seed)
        p = str(tmp_path / f"s{seed}.fq")
        with open(p, "wb") as f:
            f.write(body.encode("latin-1"))
        crashed += not _check(ref, oracle_lib, host_reader, p, f"soup{seed}")
        os.unlink(p)
    assert crashed <= 25, crashed                                # (the reference's reader crashes on a few soups; those cases prove nothing)


SPLIT_DELIMS = (" ", ";", "=", "|", "\t", "ab", "  ")


def split_lines():
    rng = random.Random(3)
    lines = ["", " ", "a", "a b", "a  b", " a b ", "x;y;;z;", "k=v", "=", "1 C1=100;C2=200", "a||b|", "|", "tab\there", "ab" * 50]
    for _ in range(300):
        lines.append("".join(rng.choice("ab ;=|\t") for _ in range(rng.randrange(0, 30))))
    return lines


def test_split_equals_reference_util_h(ref, host_util):
    lines = split_lines()
    data = ("\n".join(lines) + "\n").encode()
    for delim in SPLIT_DELIMS:
        want = ref.golden["split"][delim]
        if ref.exe is not None:
            live = subprocess.run([ref.exe, "split", delim], input=data, capture_output=True, check=True, timeout=60).stdout
            assert len(live.splitlines()) == len(lines)
            assert digest(live) == want, (delim, "the live reference no longer gives the pinned answer")
        for who in ("host", "oracle"):
            got = subprocess.run([host_util, who, "split", delim], input=data, capture_output=True, check=True, timeout=60).stdout
            assert len(got.splitlines()) == len(lines), (who, delim)
            assert digest(got) == want, (who, delim)


def overlap_cases():
    """util.h overlap() over the domain classify reaches (fEM.h:757-773: a 1000-base window clipped to the contig against a read's
    mapping clipped to the contig) and over random interval pairs; the reference asserts left < right for both intervals, so
    one-base intervals (a contig of 1000 k + 1 bases has a one-base last window: the reference aborts there) are left out"""
    rng = random.Random(9)
    cases = []
    for _ in range(3000):
        clen = rng.choice([999, 1000, 1001, 1500, 2000, 2002, 12345, 60000])
        start = rng.randrange(0, clen - 1)
        stop = min(clen - 1, start + rng.choice([1, 10, 999, 1000, 1001, 2500, 10000]))
        for pos in range(start, stop + 1, 1000):
            wi = pos // 1000
            ws, we = wi * 1000, (wi + 1) * 1000 - 1
            if we > clen:
                we = clen - 1
            if ws < we and start < stop:
                cases.append((ws, we, start, stop))
    for _ in range(3000):
        a, c = rng.randrange(0, 5000), rng.randrange(0, 5000)
        cases.append((a, a + rng.randrange(1, 3000), c, c + rng.randrange(1, 3000)))
    return cases


def test_overlap_equals_reference_util_h(ref, host_util):
    cases = overlap_cases()
    data = "".join("%d %d %d %d\n" % t for t in cases).encode()
    want = ref.golden["overlap"]
    if ref.exe is not None:
        live = subprocess.run([ref.exe, "overlap"], input=data, capture_output=True, check=True, timeout=60).stdout
        assert len(live.splitlines()) == len(cases)
        assert digest(live) == want, "the live reference no longer gives the pinned answer"
    for who in ("host", "oracle"):
        got = subprocess.run([host_util, who, "overlap"], input=data, capture_output=True, check=True, timeout=60).stdout
        assert len(got.splitlines()) == len(cases), who
        assert digest(got) == want, who
