"""CPU test of the CLI's --mods host code (metamaps_amd/csrc/host/mods_out.hpp, and the aux-field walk of bam_reader.hpp) through the small driver
tests/test_mods_out.cpp, against tests/mods_ref.py and the BAM writer of tests/bam_writer.py: the MM parser on every group shape (several codes in one
group with interleaved ML, strand - and base N dropped, U read as T, a ChEBI code, an unlisted code, the three modes, empty skip lists, an empty tag),
every malformed tag with its message, the MN mismatch; the aux walk over every BAM aux type with MM / ML first, last and absent and records that span
BGZF blocks; the 18 columns with pct at 0, 1/3, 2/3 and 1; the option refusals."""
import os
import struct
import subprocess

import pytest

import bam_writer as bw
import mods_ref

HERE = os.path.dirname(os.path.abspath(__file__))
LIST = "C+m,C+h,A+a,C+21839"
CODES = mods_ref.parse_list(LIST)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("mods_out") / "t")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", e,
                    os.path.join(HERE, "test_mods_out.cpp"), "-lz"], check=True, timeout=300)
    return e


def mm_field(text):
    return b"MMZ" + text.encode() + b"\0"


def ml_field(values, sub=b"C"):
    return b"MLB" + sub + struct.pack("<I", len(values)) + b"".join(struct.pack({b"C": "<B", b"c": "<b", b"S": "<H"}[sub], v) for v in values)


# one of every aux type (A c C s S i I f Z H and B of c C s S i I f), none of them named MM, ML or MN
OTHERS = (b"XAAq" + b"Xcc\xfe" + b"XCC\x07" + b"Xss" + struct.pack("<h", -300) + b"XSS" + struct.pack("<H", 60000) + b"Xii" + struct.pack("<i", -70000) + b"XII" + struct.pack("<I", 4000000000)
          + b"Xff" + struct.pack("<f", 1.5) + b"XZZtext with MM:Z: inside\0" + b"XHH1AE3\0" + b"".join(b"B" + t + b"B" + t + struct.pack("<I", 3) + struct.pack("<3" + f, 1, 2, 3)
                                                                                                 for t, f in ((b"c", "b"), (b"C", "B"), (b"s", "h"), (b"S", "H"), (b"i", "i"), (b"I", "I"), (b"f", "f"))))
SHAPES = [  # (name, MM text, ML values, MN or None)
    ("plain", "C+m?,0,1,0;", [1, 2, 3], None), ("two_codes", "C+mh?,0,2;A+a.,1;", [10, 20, 30, 40, 50], 12), ("chebi", "C+21839,3;", [9], None), ("unlisted", "G+o?,1;C+m,0;", [7, 8], None),
    ("minus_and_n", "C-m?,1;N+n?,0,0;C+h.,2;G-o;", [1, 2, 3, 4], None), ("u_is_t", "U+m?,0;T+g.,1;", [5, 6], None), ("empty_skips", "C+m?;A+a.;C+h;", [], None), ("empty_tag", "", [], 12),
    ("mn_mismatch", "C+m?,0;", [200], 13), ("same_code_other_strand", "C+m,0;G-m,1;", [1, 2], None), ("big_skip", "C+m?,4294967295;", [1], None),
]
BAD = [  # (name, MM field bytes, ML field bytes, MN field bytes, part of the message)
    ("bad_base", mm_field("X+m,0;"), ml_field([1]), b"", "does not start with one of"), ("no_strand", mm_field("Cm,0;"), ml_field([1]), b"", "no strand"),
    ("no_code", mm_field("C+,0;"), ml_field([1]), b"", "no code"), ("upper_code", mm_field("C+M,0;"), ml_field([1]), b"", "no code"),
    ("no_semicolon", mm_field("C+m,0"), ml_field([1]), b"", "does not end with ';'"), ("bad_skip", mm_field("C+m,x;"), ml_field([1]), b"", "skip is not a number"),
    ("skip_2_32", mm_field("C+m,4294967296;"), ml_field([1]), b"", "skip is not a number"), ("mixed_code", mm_field("C+m1,0;"), ml_field([1]), b"", "does not end with ';'"),
    ("ml_short", mm_field("C+mh,0,1;"), ml_field([1, 2, 3]), b"", "fewer than"), ("ml_long", mm_field("C+m,0;"), ml_field([1, 2]), b"", "more than"),
    ("ml_without_mm", b"", ml_field([1]), b"", "ML tag without an MM tag"), ("mm_without_ml", mm_field("C+m,0;"), b"", b"", "holds 0 bytes, fewer"),
    ("mm_type", b"MMH4143\0", b"", b"", "MM tag has type H"), ("ml_type", mm_field("C+m,0;"), ml_field([1], b"c"), b"", "not an array of type B:C"),
    ("ml_type_s", mm_field("C+m,0;"), ml_field([1], b"S"), b"", "not an array of type B:C"), ("mn_type", mm_field("C+m,0;"), ml_field([1]), b"MNZ12\0", "MN tag has type Z"),
    ("twice", mm_field("C+m,0;C+m?,1;"), ml_field([1, 2]), b"", "the code C+m is in two groups"), ("twice_combined", mm_field("C+mh,0;C+h,1;"), ml_field([1, 2, 3]), b"", "the code C+h is in two groups"),
    ("too_many", mm_field("".join("A+%d;" % (1000 + k) for k in range(256))), ml_field([]), b"", "more than 255 groups"),
]


def want_groups(mm, ml, mn, l_seq, dropped):
    g = mods_ref.parse_tags(mm, ml, mn, l_seq, CODES, dropped)
    if g is None:
        return "none"
    return "groups:" + " /".join(f" {x['base']} {x['code']} {ord(x['mode']) if x['mode'] else 0} {len(x['skips'])}" + "".join(f" {v}" for v in x["skips"] + x["ml"]) for x in g)


def run_bam(exe, path):
    p = subprocess.run([exe, "bam", path, LIST], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout.decode().splitlines()


def test_the_parser_on_every_group_shape_and_tag_position(exe, tmp_path):
    read = "ACGTACCGTTAC"
    recs, want, dropped = [], [], {}
    for k, (name, mm, ml, mn) in enumerate(SHAPES):
        mnf = b"" if mn is None else (b"MNi" + struct.pack("<i", mn), b"MNC" + struct.pack("<B", mn), b"MNs" + struct.pack("<h", mn))[k % 3]
        first = mm_field(mm) + ml_field(ml) + mnf + OTHERS
        last = OTHERS + mnf + ml_field(ml) + mm_field(mm)
        for pos, tags in (("first", first), ("last", last), ("between", OTHERS + mm_field(mm) + OTHERS + ml_field(ml) + mnf)):
            recs.append(bw.record_bytes(f"{name}_{pos}", read, 0x10 if k % 2 else 0, tags=tags))
            want.append(f"{name}_{pos} 12 | mm Z:{len(mm)} | ml B:C:{len(ml)} | mn {'none' if mn is None else mn} | " + want_groups(mm, ml, mn, len(read), dropped))
    recs.append(bw.record_bytes("absent", read, 0, tags=OTHERS)); want.append("absent 12 | mm -:0 | ml -:-:0 | mn none | none")
    recs.append(bw.record_bytes("no_aux", read, 0)); want.append("no_aux 12 | mm -:0 | ml -:-:0 | mn none | none")
    long_read = "ACGT" * 40000                                     # a record of 240 kB with 10 000 skips: it spans several BGZF blocks
    skips = [3] * 10000
    mm = "C+m?" + "".join(",%d" % s for s in skips) + ";"
    recs.append(bw.record_bytes("spans_blocks", long_read, 0, tags=OTHERS + mm_field(mm) + ml_field([k % 256 for k in range(10000)])))
    want.append(f"spans_blocks 160000 | mm Z:{len(mm)} | ml B:C:10000 | mn none | " + want_groups(mm, [k % 256 for k in range(10000)], None, 160000, dropped))
    path = str(tmp_path / "t.bam")
    bw.write_bgzf(path, bw.header_bytes() + b"".join(recs), block_bytes=4000)
    got = run_bam(exe, path)
    assert got[:-1] == want
    n_with = sum(1 for w in want if "| groups:" in w)
    assert got[-1] == f"counters {len(want)} {n_with} {dropped['minus']} {dropped['n']} 3" and dropped == {"minus": 9, "n": 3}
    by = {w.split(" ")[0]: w.split(" | ")[-1] for w in want}     # the restatement itself, by hand
    assert by["two_codes_first"] == "groups: C 0 63 2 0 2 10 30 / C 1 63 2 0 2 20 40 / A 2 46 1 1 50"
    assert by["minus_and_n_last"] == "groups: C 1 46 1 2 4" and by["u_is_t_first"] == "groups: T -1 63 1 0 5 / T -1 46 1 1 6" and by["chebi_first"] == "groups: C 3 0 1 3 9"
    assert by["empty_tag_first"] == "groups:" and by["mn_mismatch_first"] == "none" and by["empty_skips_first"] == "groups: C 0 63 0 / A 2 46 0 / C 1 0 0"


def test_every_malformed_tag_and_its_message(exe, tmp_path):
    recs = [bw.record_bytes(name, "ACCA", 0, tags=OTHERS + mmf + mlf + mnf) for name, mmf, mlf, mnf, _ in BAD]
    path = str(tmp_path / "bad.bam")
    bw.write_bgzf(path, bw.header_bytes() + b"".join(recs))
    got = run_bam(exe, path)
    for (name, mmf, mlf, mnf, what), g in zip(BAD, got):
        assert g.startswith(name + " 4 |") and " | error: " in g and what in g.split(" | error: ")[1], (name, g)
        if mmf.startswith(b"MMZ") and mlf.startswith(b"MLBC") and not mnf:
            with pytest.raises(ValueError):
                mods_ref.parse_tags(mmf[3:-1].decode(), list(mlf[8:]), None, 4, CODES)
    assert got[-1].startswith(f"counters {len(BAD)} 0 ")
    # aux fields that run over the record's end, or of an unknown type, are the reader's error
    for k, tags in enumerate((b"MMZC+m,0;", b"XYB", b"XYBC" + struct.pack("<I", 9) + b"\1\2", b"XYi\1\2", b"XY?\1", b"XYBA" + struct.pack("<I", 1) + b"q", b"XY")):
        bw.write_bgzf(path, bw.header_bytes() + bw.record_bytes("r", "ACCA", 0, tags=tags))
        assert run_bam(exe, path) == [f"bam error: {path}: corrupt BAM record (aux fields) of read r"], (k, tags)


def test_the_18_columns(exe):
    K = mods_ref.key
    rows = [(0, 5, 1, 0, 0, 3, 0, 2), (0, 5, 1, 1, 1, 2, 0, 2), (1, 0, -1, 2, 2, 1, 0, 0), (1, 4294967295, -1, 3, 7, 0, 0, 1), (1, 9, 1, 0, 0xFFFFFFFF, 0, 2 * 0xFFFFFFFF, 0)]
    text = "chrA chrB\n" + "".join(f"{K(c, pos, s, k)} {a} {b} {o} {f}\n" for c, pos, s, k, a, b, o, f in rows)
    p = subprocess.run([exe, "text", LIST], input=text.encode(), capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == mods_ref.bedmethyl_text(rows, ["chrA", "chrB"], [c for _, c in CODES])
    lines = [l.split("\t") for l in p.stdout.decode().splitlines()]
    assert all(len(l) == 18 for l in lines) and [l[10] for l in lines] == ["0.00", "33.33", "66.67", "100.00", "33.33"]
    assert lines[1] == ["chrA", "5", "6", "h", "3", "+", "5", "6", "255,0,0", "3", "33.33", "1", "2", "0", "0", "2", "0", "0"]
    assert lines[3][:6] == ["chrB", "4294967295", "4294967296", "21839", "7", "-"]


def test_the_options(exe):
    def run(*args):
        p = subprocess.run([exe, "opts"] + list(args), capture_output=True, timeout=60)
        return p.returncode, p.stdout.decode().strip(), p.stderr.decode().strip()
    assert run() == (0, "0 204 1", "")
    assert run("mods=" + LIST) == (0, "4 C:m C:h A:a C:21839 204 1", "")
    assert run("mods=T+abc", "mod-min-ml=0", "mod-min-coverage=999999999") == (0, "1 T:abc 0 999999999", "")
    assert run("mods=A+a", "mod-min-ml=255") == (0, "1 A:a 255 1", "")
    for args, what in ((["mods="], "--mods takes 1 to 4"), (["mods=C+m,"], "--mods takes 1 to 4"), (["mods=C+m,C+h,A+a,T+g,G+x"], "--mods takes 1 to 4"), (["mods=N+m"], "--mods takes 1 to 4"),
                       (["mods=c+m"], "--mods takes 1 to 4"), (["mods=C-m"], "--mods takes 1 to 4"), (["mods=C+M"], "--mods takes 1 to 4"), (["mods=C+m1"], "--mods takes 1 to 4"),
                       (["mods=C+"], "--mods takes 1 to 4"), (["mods=C+m,C+m"], "--mods: the item C+m is given twice"), (["mods=C+m,A+a,C+m"], "given twice"),
                       (["mod-min-ml=5"], "--mod-min-ml needs --mods"), (["mod-min-coverage=5"], "--mod-min-coverage needs --mods"),
                       (["mods=C+m", "mod-min-ml=256"], "from 0 to 255"), (["mods=C+m", "mod-min-ml=-1"], "from 0 to 255"), (["mods=C+m", "mod-min-ml=1e2"], "from 0 to 255"),
                       (["mods=C+m", "mod-min-coverage=0"], "from 1 to"), (["mods=C+m", "mod-min-coverage=x"], "from 1 to"), (["mods=C+m", "mod-min-coverage="], "from 1 to")):
        rc, out, err = run(*args)
        assert rc == 1 and out == "" and what in err, (args, err)
