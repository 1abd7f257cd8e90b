#!/usr/bin/env python3
"""Regenerates tests/golden/ref_golden.json: what the reference's own code answers on the inputs of tests/test_ref_host.py and
of the murmur cross-check of tests/test_oracle_golden.py, as sha256 digests (first 24 hex digits), so that those tests need
nothing outside the repository.

  kseq     per input (curated layout, the same layout gzipped, byte soup seed): [digest of `ref_host kseq` output, number of
           records], or null where the reference's reader crashes on it
  split    per delimiter: digest of `ref_host split DELIM` output
  overlap  digest of `ref_host overlap` output
  murmur   digest of the reference header's hashes of the cases, as little-endian uint32

Needs oracle/_ref (make -C oracle ref, which needs the reference tree).  Run from the repository root:
python tests/golden/make_ref_golden.py"""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_oracle_golden as tog  # noqa: E402
import test_ref_host as trh  # noqa: E402


def main():
    exe, lib = trh.REF, os.path.join(ROOT, "oracle", "_ref", "libref_murmur.so")
    if not (os.path.exists(exe) and os.path.exists(lib)):
        sys.exit("oracle/_ref is not built: make -C oracle ref")
    out = {"kseq": {}}

    def kseq(key, data):
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "in.fq")
            with open(p, "wb") as f:
                f.write(data)
            k = trh._kseq(exe, p)
        out["kseq"][key] = [trh.kseq_digest(*k), len(k[0])] if k else None

    for name, text in sorted(trh.LAYOUTS.items()):
        data = text.encode("latin-1")
        kseq(name, data)
        with tempfile.TemporaryDirectory() as d:               # the .gz input of the test: gzip.open over the same bytes
            p = os.path.join(d, "in.fq.gz")
            with gzip.open(p, "wb") as g:
                g.write(data)
            k = trh._kseq(exe, p)
        out["kseq"][name + ".gz"] = [trh.kseq_digest(*k), len(k[0])] if k else None
    for seed in trh.SOUP_SEEDS:
        kseq(f"soup{seed}", trh.soup(seed).encode("latin-1"))

    data = ("\n".join(trh.split_lines()) + "\n").encode()
    out["split"] = {d: trh.digest(subprocess.run([exe, "split", d], input=data, capture_output=True, check=True).stdout) for d in trh.SPLIT_DELIMS}
    data = "".join("%d %d %d %d\n" % t for t in trh.overlap_cases()).encode()
    out["overlap"] = trh.digest(subprocess.run([exe, "overlap"], input=data, capture_output=True, check=True).stdout)

    ref = C.CDLL(lib)
    ref.ref_kmer_hash.restype = C.c_uint32
    out["murmur"] = tog.murmur_digest([ref.ref_kmer_hash(s, k) for s, k in tog.murmur_cases()])

    with open(os.path.join(HERE, "ref_golden.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out['kseq'])} reader inputs ({sum(v is None for v in out['kseq'].values())} crash the reference), "
          f"{len(out['split'])} split delimiters, overlap, murmur")


if __name__ == "__main__":
    main()
