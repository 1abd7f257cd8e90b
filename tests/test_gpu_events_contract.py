"""What mm_pileup_events_q, mm_vcf_events_q and mm_mod_events share is one pipeline (metamaps_amd/csrc/mm_events.hpp); what a caller sees of each must stay
its own.  Per format, on one job of its *_cases.py: the exact text of the parameter's refusal with its status and a NULL handle; the checks of the sets come
before the parameter's; and the stage line under the format's timing variable, as tools/edit_kernel_stats.py reads it, printed by a fresh child process."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

MS = r"\d+\.\d{3}"
STAGES = rf"events: upload {MS} count {MS} scan {MS} emit {MS} sort {MS} reduce {MS} ms; "
# kind -> the parameter's name and a value beyond its range, the refusal, the entry point's name, the timing variable, the line behind the stage times, bytes per row
FORMATS = {
    "pileup": ("min_base_quality", 94, "mm_pileup_events_q: min_base_quality is not in [0, 93]", "mm_pileup_events", "MM_PILEUP_TIMING",
               r"(\d+) jobs, (\d+) runs, (\d+) events, (\d+) pairs, (\d+) B fetched", 12),
    "vcf": ("min_base_quality", 94, "mm_vcf_events_q: min_base_quality is not in [0, 93]", "mm_vcf_events", "MM_VCF_TIMING",
            r"(\d+) jobs, (\d+) runs, (\d+) events \((\d+) indels\), (\d+) pairs, (\d+) B fetched", 20),
    "mod": ("min_ml", 256, "mm_mod_events: min_ml is not in [0, 255]", "mm_mod_events", "MM_MODS_TIMING",
            r"(\d+) jobs, (\d+) runs, (\d+) events, (\d+) pairs, (\d+) B fetched", 12),
}


def world(kind):
    """(contigs, the one job, its modification groups or None)"""
    if kind == "pileup":
        import pileup_cases
        contigs, jobs = pileup_cases.built_world()
        return contigs[:1], jobs["x_at_0"], None                   # one mismatch: one event
    if kind == "vcf":
        import vcf_cases
        contigs, jobs = vcf_cases.built_world()
        return contigs[:1], jobs["tri_del_1_f"], None              # one deletion between = runs: one indel
    import mods_cases
    contigs, jobs = mods_cases.event_world()
    return contigs[:1], jobs["fwd"], jobs["fwd"]["groups"]


def arrays(j):
    return dict(read=[0], strand=[j["strand"]], contig=[j["c"]], dist=[j["d"]], first=[j["first"]], op_off=[0, len(j["runs"])], ops=j["runs"], use=[1])


def events(ctx, kind, reads, ref, j, **param):
    return getattr(ctx, kind + "_events")(reads, ref, **arrays(j), **param)


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", FORMATS)
def test_refusals_keep_their_text_and_their_order(ctx, kind):
    from metamaps_amd import capi
    name, beyond, text, who, _, _, _ = FORMATS[kind]
    contigs, j, groups = world(kind)
    assert j["c"] == 0
    reads, ref = ctx.seqset([j["read"]], mods=[groups] if groups else None), ctx.seqset(contigs)
    staged = C.c_void_p()                                          # a read set that is made and never uploaded
    assert capi.lib().mm_seqset_create(ctx.h, C.byref(staged)) == 0 and staged.value
    try:
        assert capi.lib().mm_seqset_add(staged, bytes(j["read"]), len(j["read"])) == 0
        assert len(events(ctx, kind, reads, ref, j)[0]) > 0
        with pytest.raises(capi.MMError) as e:
            events(ctx, kind, reads, ref, j, **{name: beyond})
        assert e.value.status == capi.MM_ERR_ARG and capi.lib().mm_last_error(ctx.h).decode() == text
        assert getattr(ctx, f"last_{kind}_handle") is None
        with pytest.raises(capi.MMError) as e:                     # both wrong: the sets are asked first
            events(ctx, kind, capi.SeqSet(ctx, staged), ref, j, **{name: beyond})
        assert e.value.status == -4 and capi.lib().mm_last_error(ctx.h).decode() == who + ": a sequence set is not uploaded"
        assert getattr(ctx, f"last_{kind}_handle") is None
    finally:
        capi.lib().mm_seqset_destroy(staged)
        reads.close(); ref.close()


def child():
    """one events call per format; the rows of each table as one JSON line (the stage lines go to stderr)"""
    from metamaps_amd import capi
    ctx = capi.Context(0)
    rows = {}
    for kind in FORMATS:
        contigs, j, groups = world(kind)
        reads, ref = ctx.seqset([j["read"]], mods=[groups] if groups else None), ctx.seqset(contigs)
        rows[kind] = len(events(ctx, kind, reads, ref, j)[0])
        reads.close(); ref.close()
    ctx.close()
    print(json.dumps(rows))


def test_the_timing_lines():
    env = dict(os.environ, **{f[4]: "1" for f in FORMATS.values()})
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    for kind, (_, _, _, _, var, tail, row_bytes) in FORMATS.items():
        lines = [ln for ln in p.stderr.splitlines() if ln.startswith(var + " events:")]
        assert len(lines) == 1, (kind, p.stderr)
        m = re.fullmatch(var + " " + STAGES + tail, lines[0])
        assert m, lines[0]
        f = [int(x) for x in m.groups()]
        n_runs = len(world(kind)[1]["runs"])
        assert f[0] == 1 and f[1] == n_runs and f[2] >= f[-2] == rows[kind] > 0 and f[-1] == rows[kind] * row_bytes, (kind, lines[0])
        if kind == "vcf":
            assert f[3] == 1, lines[0]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child()
