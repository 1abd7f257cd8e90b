"""Base modifications (the MM/ML tags of a read, SAM tags specification, "Base modifications") counted per reference position, restated plainly: loops
over bases and dicts of counts.  It shares no code with metamaps_amd/csrc/mm_mods_core.hpp; tests/test_mods_core.py holds the header's host form to it,
tests/test_gpu_seqset_mods.py and tests/test_gpu_mod_events.py the device.

A group is a dict with base (one of "ACGT"), code (the index 0..3 of its code in the list of asked codes, -1 for a code that is not in the list),
mode ("." , "?" or "" for absent), skips (the MM numbers) and ml (one byte per skip): one code per group, a group of several codes is split before.
A job is pileup_ref.py's dict (read, strand, c, first, runs, d, use) with `plane`, the (who, prob) of its read, or None for a read without one."""

WHO_NONE, WHO_CANONICAL, WHO_OTHER, WHO_CODE0 = 0, 1, 2, 3
CLASS_CANONICAL, CLASS_FAIL, CLASS_OTHER, CLASS_CODE0 = 0, 1, 2, 3
DEFAULT_MIN_ML = 204
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


class DataError(Exception):
    """a group names an occurrence of its base that the read does not have; .group is the lowest such group of the read"""
    def __init__(self, group):
        super().__init__(f"group {group}")
        self.group = group


def parse_list(text):
    """--mods LIST: 1 to 4 items B+code -> [(base, code)]; ValueError otherwise"""
    items = text.split(",")
    if not 1 <= len(items) <= 4:
        raise ValueError(text)
    out = []
    for it in items:
        if len(it) < 3 or it[0] not in "ACGT" or it[1] != "+" or not (it[2:].isdigit() or (it[2:].isalpha() and it[2:].islower() and it[2:].isascii())):
            raise ValueError(it)
        if (it[0], it[2:]) in out:
            raise ValueError("duplicate " + it)
        out.append((it[0], it[2:]))
    return out


def parse_tags(mm, ml, mn, l_seq, codes, dropped=None):
    """the groups of a read's MM text and ML bytes (mn: its MN value or None) for the asked codes [(base, code)], or None for a read that is dropped (its
    MN differs from l_seq); ValueError for malformed tags.  dropped: a dict that counts the groups of strand - ("minus") and of base N ("n")"""
    import re
    if not re.fullmatch(r"([ACGTUN][-+]([a-z]+|[0-9]+)[.?]?(,[0-9]+)*;)*", mm):
        raise ValueError("syntax")
    groups, seen, at = [], set(), 0
    for m in re.finditer(r"([ACGTUN])([-+])([a-z]+|[0-9]+)([.?]?)((?:,[0-9]+)*);", mm):
        base, strand, code, mode, tail = m.groups()
        base = "T" if base == "U" else base
        names = [code] if code.isdigit() else list(code)
        skips = [int(x) for x in tail.split(",")[1:]]
        if any(x >= 1 << 32 for x in skips) or at + len(skips) * len(names) > len(ml):
            raise ValueError("skips")
        for c, name in enumerate(names):
            if (base, strand, name) in seen:
                raise ValueError("twice")
            seen.add((base, strand, name))
            if strand == "-" or base == "N":
                if dropped is not None:
                    dropped["minus" if strand == "-" else "n"] = dropped.get("minus" if strand == "-" else "n", 0) + 1
                continue
            groups.append(dict(base=base, code=codes.index((base, name)) if (base, name) in codes else -1, mode=mode, skips=skips,
                               ml=[ml[at + j * len(names) + c] for j in range(len(skips))]))
        at += len(skips) * len(names)
    if at != len(ml) or len(groups) > 255:
        raise ValueError("ML length")
    return None if mn is not None and mn != l_seq else groups


def ordinals(g):
    """the 1-based occurrences of its base that group g names"""
    out, o = [], 0
    for s in g["skips"]:
        o += int(s) + 1
        out.append(o)
    return out


def plane(read, groups):
    """(who, prob), one byte per base each, of a read as its set holds it"""
    letters = bytes(read).decode("latin-1").upper()
    for k, g in enumerate(groups):
        assert len(g["skips"]) == len(g["ml"]) and g["base"] in "ACGT" and -1 <= g["code"] <= 3 and g["mode"] in (".", "?", "")
        o = ordinals(g)
        if o and o[-1] > letters.count(g["base"]):
            raise DataError(k)
    named = [dict(zip(ordinals(g), g["ml"])) for g in groups]
    seen = {b: 0 for b in "ACGT"}
    who, prob = bytearray(len(letters)), bytearray(len(letters))
    for i, ch in enumerate(letters):
        if ch not in seen:
            continue
        seen[ch] += 1
        ps = []                                                     # (p, group) in MM order
        for k, g in enumerate(groups):
            if g["base"] != ch:
                continue
            if seen[ch] in named[k]:
                ps.append((int(named[k][seen[ch]]), k))
            elif g["mode"] != "?":
                ps.append((0, k))
        if not ps:
            continue
        pc = 255 - min(255, sum(p for p, _ in ps))
        best = max(p for p, _ in ps)
        star = next(k for p, k in ps if p == best)
        if pc >= best:
            who[i], prob[i] = WHO_CANONICAL, pc
        else:
            code = groups[star]["code"]
            who[i], prob[i] = (WHO_CODE0 + code if code >= 0 else WHO_OTHER), best
    return bytes(who), bytes(prob)


def key(contig, pos, strand, cls):
    return contig << 36 | pos << 4 | (1 if strand < 0 else 0) << 3 | cls


def unkey(k):
    k = int(k)
    return k >> 36, (k >> 4) & 0xFFFFFFFF, -1 if k >> 3 & 1 else 1, k & 7


def contributes(j):
    return j.get("use", 1) != 0 and j["d"] >= 0


def events(j, min_ml=DEFAULT_MIN_ML):
    """the events of one contributing alignment as (contig, pos, strand, class), in the order of the walk"""
    if j.get("plane") is None:
        return []
    who, prob = j["plane"]
    m = len(j["read"])
    assert len(who) == m and len(prob) == m
    r, i, out = j["first"], 0, []
    for w in j["runs"]:
        n, op = int(w) >> 4, int(w) & 15
        if op == 7:
            for t in range(n):
                s = i + t if j["strand"] > 0 else m - 1 - (i + t)
                if who[s] != WHO_NONE:
                    cls = CLASS_FAIL if prob[s] < min_ml else {WHO_CANONICAL: CLASS_CANONICAL, WHO_OTHER: CLASS_OTHER}.get(who[s], who[s])
                    out.append((j["c"], r + t, j["strand"], cls))
            r += n; i += n
        elif op == 8:
            r += n; i += n
        elif op == 2:
            r += n
        elif op == 1:
            i += n
        else:
            raise ValueError(w)
    assert i == m
    return out


def table(jobs, min_ml=DEFAULT_MIN_ML):
    """{key: count} over the contributing jobs"""
    t = {}
    for j in jobs:
        if contributes(j):
            for e in events(j, min_ml):
                t[key(*e)] = t.get(key(*e), 0) + 1
    return t


def merged(pairs):
    t = {}
    for k, c in pairs:
        t[int(k)] = t.get(int(k), 0) + int(c)
    return t


def rows(t, contig_bytes, code_base, min_coverage=1):
    """[(contig, pos, strand, k, n_mod, n_canonical, n_other_mod, n_fail)] of a merged table; code_base: the base letter of every listed code"""
    sites = {}
    for k, n in t.items():
        c, pos, strand, cls = unkey(k)
        sites.setdefault((c, pos, 0 if strand > 0 else 1), {})[cls] = n
    out = []
    for (c, pos, minus) in sorted(sites):
        cnt = sites[(c, pos, minus)]
        b = chr(contig_bytes[c][pos]).upper()
        if b not in _COMP:
            continue
        if minus:
            b = _COMP[b]
        for k, base in enumerate(code_base):
            if base != b:
                continue
            n_mod = cnt.get(CLASS_CODE0 + k, 0)
            n_canon = cnt.get(CLASS_CANONICAL, 0)
            n_other = cnt.get(CLASS_OTHER, 0) + sum(cnt.get(CLASS_CODE0 + o, 0) for o in range(len(code_base)) if o != k)
            if n_mod + n_canon + n_other >= min_coverage:
                out.append((c, pos, -1 if minus else 1, k, n_mod, n_canon, n_other, cnt.get(CLASS_FAIL, 0)))
    return out


def bedmethyl_text(rws, cname, code_name):
    """PREFIX.bedmethyl: modkit's 18 tab-separated columns, no header"""
    out = []
    for c, pos, strand, k, n_mod, n_canon, n_other, n_fail in rws:
        valid = n_mod + n_canon + n_other
        pct = "%.2f" % (100.0 * n_mod / valid) if valid else "0.00"
        out.append("\t".join(str(x) for x in (cname[c], pos, pos + 1, code_name[k], valid, "+" if strand > 0 else "-", pos, pos + 1, "255,0,0", valid, pct, n_mod, n_canon, n_other,
                                                0, n_fail, 0, 0)) + "\n")
    return "".join(out).encode("latin-1")
