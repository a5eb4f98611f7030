"""The generation calls of the resident route's recursion (include/parsnp_mum.h: pm_store_search / _search_beside, pm_store_validate,
pm_store_order_check), call by call against the sequential work list of tests/gencalls.py, in the kernel emulation (tests/emu: one
host thread plays every lane of ClustersDisjoint, ClusterExtents .. ClusterDefer, ReaderMark .. ReaderLook, ClusterValidate,
StageGate, OutsideWriteCheck and the order check's kernels).  tests/test_gpu_gen_calls.py runs the same checks on the device.

Per call: the candidates of every searched region, row by row; info[] and pm_store_info of every decided row; the layout bit for
bit; the children through their listed order; done[] as properties (gencalls.EngineSide.validate).  At the end, where no trouble
was reported, the run equals the reference's work list: the reference's order could not be seen.  Variants: every generation as ONE
cluster (the serial extreme: done[] partial in nearly every call, clusters of more than kPieces regions), two stages in one call
with a first seed that pushes no child and one that does, the tunes "stage_gate" and "cluster_unsure", done == NULL on a list with a
waiting cluster and on one with a partial cluster, the refusals, and the rearranged cases with the wavefronts of one launch at a
time running last to first.

Every case asserts its floors from the restatement alone (test_floors)."""
import os
import re
import subprocess

import numpy as np
import pytest

import gencalls as G
from parsnp_amd.binding import Lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REARRANGED = ["rearranged8", "rearranged8_margin", "inverted70"]
ORDER = list(G.ORDER_ROWS)      # the cases on which a reader runs beside a marker and the order check has to decide
REVERSED_LAUNCHES = ["cluster_validate", "cluster_extents", "marker_look", "reader_mark"]


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


_runs = {}


def run(lib, case, **kw):
    """one session per (library, case, variant), shared by the tests"""
    key = (lib.path, case, tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = G.run_case(lib, case, **kw)
    return _runs[key]


# ------------------------------------------------------------------------------------------------------------------ the checks
def check_floors(case):
    """the case takes the paths it is for, by the restatement alone: lowering q or raising the anchor call's minimum length until a
    path is lost turns this red"""
    name, ams, q, recorded = G.CASES[case]
    ref = G.reference(case)
    got = dict(zip(("generations", "with_cands", "without", "trimmed", "kept", "at_q", "dups", "met", "reverse_outside"), ref.numbers))
    assert ref.open_ties == 0, "a tie run in which two regions have candidates: the reference's unstable sort would decide"
    assert ref.work.stats.long_outside == 0, "a reverse candidate of more than 64 bases with a member outside its region ends the route"
    for k, v in G.FLOORS.items():
        assert got[k] >= v, "%s: %s = %d, the floor is %d (%s)" % (case, k, got[k], v, got)
    if case in REARRANGED:
        for k, v in G.REARRANGED_FLOORS.items():
            assert got[k] >= v, "%s: %s = %d, the floor is %d (%s)" % (case, k, got[k], v, got)
    assert ref.order_free, "the accepted rows of the restatement's generation run differ from do_work(): the order check must answer non-zero, say so in the case"
    assert ref.order_rows >= G.ORDER_ROWS.get(case, 0), "no row that is trimmed differently in generation order and in list order"
    assert ref.side.by_margin >= G.MARGIN_FLOOR.get(case, 0), "no reader and marker of two clusters one base apart"
    assert got["dups"] == recorded[6] == 0, "the restatement drops a duplicate child on this set: give it a floor"
    assert ref.numbers == recorded, "%s: the restatement gives %s, CASES records %s" % (case, ref.numbers, recorded)


def check_generations(lib, case, **kw):
    """every call of a whole run (the comparisons are made while it runs: gencalls.EngineSide), then the end state"""
    r = run(lib, case, **kw)
    ref = G.reference(case, kw.get("rotate", 0))
    what = "%s %s" % (case, kw or "")
    assert r.left is None, "%s: the former left the route: %s" % (what, r.left)
    assert r.finished and r.order == 0, "%s: trouble %d, order check %s; the restatement's accepted rows do not depend on the order" % (what, r.trouble, r.order)
    if case in ORDER:
        assert not any(c["exact"] for c in r.calls), what + ": the exact cluster test ran; the case is for the calls that pass the collinear test"
    assert len(r.calls) >= 3 and sum(1 for c in r.calls if c["kids"]) >= 2, what
    if case.startswith("collinear"):
        assert r.trouble == 0 and r.order == 0, "%s: trouble %d, order check %s on a collinear set" % (what, r.trouble, r.order)
        assert not any(c["deferred"] for c in r.calls), what + ": a cluster waits on a collinear set"
    if r.finished and r.order == 0:
        G.same_end_state(r, ref, what)
    return r


def check_end_state(lib):
    """the rearranged sets: no trouble implies the reference's work list (check_generations), and at least one of them gets there"""
    ends = [run(lib, case) for case in REARRANGED]
    assert any(r.finished and r.order == 0 for r in ends), [(r.trouble, r.order) for r in ends]
    assert all(sum(c["deferred"] for c in r.calls) >= 1 and sum(c["met"] for c in r.calls) >= 1 for r in ends), "no cluster waited"
    assert any(c["largest"] > G.K_PIECES and len(c["done"]) > 1 for r in ends for c in r.calls), "no cluster of more than kPieces regions beside another"


def check_coarse(lib, case):
    r = check_generations(lib, case, coarse=True)
    assert all(len(c["done"]) == 1 for c in r.calls)
    assert sum(c["partial"] for c in r.calls) >= 3 and max(c["largest"] for c in r.calls) > G.K_PIECES, [(c["partial"], c["largest"]) for c in r.calls]
    assert r.finished and r.order == 0, "one cluster per generation is the serial order: trouble %d, order check %s" % (r.trouble, r.order)


def pushing_seed(case, pushes):
    """the first seed of the case's list whose processing FIRST pushes a child / pushes none, by the restatement"""
    name, ams, q, _ = G.CASES[case]
    base = G.reference(case).base
    for i, s in enumerate(G.reference(case).seeds):
        m = base.fork()
        t = s.twin()
        m.search_region(t)
        if bool(m.validate_region(t, q)) == pushes:
            return i
    raise AssertionError("no such seed")


def check_two_stages(lib, case="collinear6"):
    """stage_first = 1 with a first seed that pushes no child (the second stage runs: everything as in one-stage calls) and with one
    that does (it does not: only the first seed is processed, the caller forms the generation again); "stage_gate" forces the second
    outcome on the first list; the end state is the work list's every time"""
    quiet, loud = pushing_seed(case, False), pushing_seed(case, True)
    for rotate, tune, ran in ((quiet, None, 1), (loud, None, 0), (quiet, {"stage_gate": 1}, 0)):
        r = check_generations(lib, case, two_stage=True, rotate=rotate, **({"tune": tuple(tune.items())} if tune else {}))
        c = r.calls[0]
        assert c["stage_first"] == 1 and c["second_ran"] == ran, (rotate, tune, c["second_ran"])
        assert c["done"][0] == 1 and (ran or not any(c["done"][1:])), c["done"]
        assert ran or (c["kids"] > 0) == (rotate == loud), c      # (the children of a first stage alone: the first seed's)
        assert r.finished and r.order == 0
        one = check_generations(lib, case, rotate=rotate)
        assert one.model.by_region() == r.model.by_region(), "two stages in one call and one stage per call end differently"
        if ran:      # generation 0 and 1 of the one-stage run in one call: the same rows, the same children
            assert r.trace[0][3] == one.trace[1][3], "the layout after the two-stage call differs from the one after generations 0 and 1"


def check_cluster_unsure(lib, case):
    """"cluster_unsure": the collinear test reports failure, the exact test must find the clusters disjoint: nothing changes"""
    plain = check_generations(lib, case)
    r = check_generations(lib, case, tune=(("cluster_unsure", 1),))
    assert all(c["exact"] for c in r.calls if len(c["done"]) - c["stage_first"] > 1)
    assert sum(c["timing"].get("exact_cluster_tests", 0) for c in r.calls) >= 2, [c["timing"].get("exact_cluster_tests") for c in r.calls]
    assert not any(c["timing"].get("exact_cluster_tests", 0) for c in plain.calls)
    assert r.trace == plain.trace, "the exact cluster test changes done[], info[], the children or the layout of a collinear set"


def check_null_done(lib, case="rearranged8"):
    """done == NULL on the list of a call that left a cluster waiting (trouble bit 3) and of one that stopped inside a cluster (bit 0);
    rows, children and layout as with done[] given"""
    plain = run(lib, case)
    waits = next(i for i, c in enumerate(plain.calls) if c["deferred"])
    stops = next(i for i, c in enumerate(plain.calls) if c["partial"] and not c["deferred"])
    for at, bit in ((waits, G.TR_DEFERRED), (stops, G.TR_PARTIAL)):
        r = run(lib, case, null_done_at=at, null_expect=tuple(plain.calls[at]["done"]), stop_after=at + 1)
        assert r.calls[at]["trouble"] == bit, "done == NULL at call %d: trouble %d, expected %d" % (at, r.calls[at]["trouble"], bit)
        assert r.trace[at][1:] == plain.trace[at][1:], "done == NULL changes info[], the children or the layout"


def check_refusals_and_lists(lib, case="collinear6"):
    """after a finished run, on the open session: the refusals of pm_store_validate (PM_EINVAL, the session keeps working), and
    pm_store_search on a list with a region without candidates in the middle, ids in descending order, n = 0, through both forms"""
    seen = {}

    def then(st, side, r):
        m = side.m
        regs = [x for x in m.processed if x.eid is not None]
        full = [x for x in regs if x.cnt > 0]
        hi, lo = max(full, key=lambda x: x.eid), min(full, key=lambda x: x.eid)
        trio = [hi, next(x for x in regs if x.cnt == 0 and lo.eid < x.eid < hi.eid), lo]      # ids in descending order, the middle one without candidates
        ids, row0, cnt = [x.eid for x in trio], [x.row0 for x in trio], [x.cnt for x in trio]
        bad = [("cluster_first[0] != 0", dict(cluster_first=[1, 3])), ("cluster_first[n_clusters] != n_regions", dict(cluster_first=[0, 2])),
               ("stage_first >= n_clusters", dict(cluster_first=[0, 3], stage_first=1)), ("a row range past the store", dict(cluster_first=[0, 3], row0=[row0[0], row0[1], st.rows_total - cnt[2] + 1])),
               ("a region id past the region store", dict(cluster_first=[0, 3], ids=[ids[0], ids[1], 1 << 30]))]
        before = st.layout()
        for what, kw in bad:
            a = st.validate(kw.get("ids", ids), kw.get("row0", row0), cnt, kw["cluster_first"], 3, 99, kw.get("stage_first", 0))
            assert a.rc == G.PM_EINVAL, "%s: return code %d" % (what, a.rc)
        assert all(np.array_equal(x, y) for x, y in zip(before, st.layout())), "a refused call changed the layout"
        for beside in (False, True):
            for x in trio:
                x.row0 = None
            total = st.rows_total
            rc, first, off, calls = st.search([x.eid for x in trio], [G.region_minsize(x.slength) for x in trio], beside=beside)
            st.check(rc)
            assert first == total and off[1] == off[2] and off[1] > 0 and off[3] > off[2] and calls == (1 if beside else None), (first, total, off, calls)
            side.compare_search(trio, [G.region_minsize(x.slength) for x in trio], first, off)
            rc, first, off, calls = st.search([], [], beside=beside)
            assert rc == G.PM_OK and first == st.rows_total and off[0] == 0 and calls == (1 if beside else None), (rc, first, st.rows_total, off, calls)
        assert st.order_check() == 0      # the session keeps working
        seen["done"] = True
    G.run_case(lib, case, then=then)
    assert seen.get("done")


def check_reversed(lib, case, launch):
    """the wavefronts of one launch last to first (tests/emu/engine_emu.cpp: PM_EMU_REVERSE_WAVES): the clusters that run together are
    claimed to be disjoint, so done[], info[], the children and the layout must not change"""
    plain = run(lib, case)
    os.environ["PM_EMU_REVERSE_WAVES"] = launch
    try:
        r = G.run_case(lib, case)
    finally:
        os.environ.pop("PM_EMU_REVERSE_WAVES", None)
    assert len(r.trace) == len(plain.trace)
    for i, (a, b) in enumerate(zip(r.trace, plain.trace)):
        for what, x, y in zip(("done[]", "info[]", "the children", "the layout"), a, b):
            assert x == y, "%s with the wavefronts of %s reversed: %s of call %d changes" % (case, launch, what, i)
    assert (r.trouble, r.order) == (plain.trouble, plain.order)


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", list(G.CASES))
def test_floors(cpu_checkers, case):
    check_floors(case)


@pytest.mark.parametrize("case", list(G.CASES))
def test_generations(lib, case):
    check_generations(lib, case)


def test_end_state(lib):
    check_end_state(lib)


@pytest.mark.parametrize("case", list(G.CASES))
def test_one_cluster_per_generation(lib, case):
    check_coarse(lib, case)


def test_two_stages(lib):
    check_two_stages(lib)


@pytest.mark.parametrize("case", ["collinear70", "collinear131"])
def test_cluster_unsure(lib, case):
    check_cluster_unsure(lib, case)


def test_null_done(lib):
    check_null_done(lib)


def test_refusals_and_lists(lib):
    check_refusals_and_lists(lib)


@pytest.mark.parametrize("launch", REVERSED_LAUNCHES)
@pytest.mark.parametrize("case", REARRANGED)
def test_reversed_wavefronts(lib, case, launch):
    check_reversed(lib, case, launch)


@pytest.mark.parametrize("case", ORDER)
def test_reader_beside_marker_reversed(lib, case):
    """the clusters of every call last to first: the reader now runs AFTER the marker beside it, its rejected row is trimmed otherwise
    (not compared), every accepted row, child and layout bit is the same and the order check still answers 0"""
    check_reversed(lib, case, "cluster_validate")


def test_generator_matches_the_header():
    """kPieces, the PM_ST_* bits, the PM_ROW_* bits and the trouble bits as the sources have them"""
    eng = os.path.join(ROOT, "parsnp_amd", "csrc", "engine")
    kernels = open(os.path.join(eng, "store_kernels.h")).read()
    core = open(os.path.join(eng, "engine_core.h")).read()
    header = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    assert int(re.search(r"constexpr int kPieces = (\d+);", kernels).group(1)) == G.K_PIECES
    bits = {k: int(v) for k, v in re.findall(r"#define (PM_(?:ST|ROW)_[A-Z]+) (\d+)u", header)}
    assert (bits["PM_ST_BUILT"], bits["PM_ST_OK"], bits["PM_ST_ACCEPTED"]) == (G.ST_BUILT, G.ST_OK, G.ST_ACCEPTED)
    assert (bits["PM_ROW_BAD"], bits["PM_ROW_OUTSIDE"], bits["PM_ROW_REVERSE"]) == (G.ROW_BAD, G.ROW_OUTSIDE, G.ROW_REVERSE)
    assert int(re.search(r"#define PM_EINVAL \((-\d+)\)", header).group(1)) == G.PM_EINVAL
    # bits 0 and 3: what a caller without done[] is told (engine_core.h); bits 1 and 2: what ClusterValidate raises (store_kernels.h)
    m = re.search(r"\*trouble \|= done_h\[\(size_t\)cl\] == 0 \? (\d+)u : (\d+)u;", core)
    assert (int(m.group(1)), int(m.group(2))) == (G.TR_DEFERRED, G.TR_PARTIAL)
    raised = {int(x) for x in re.findall(r"atomic_or32\(trouble, (\d+)u\)", kernels)}
    assert raised == {G.TR_REVERSE, G.TR_LIMIT}, raised
    assert re.search(r"bit 1 \(2\).*\n.*\n.*\n.*bit 2 \(4\)", header) and "bits 0 (1) and 3 (8)" in header


def test_sanitized_program(lib, tmp_path):
    """tests/emu/gen_calls_check.cpp: the calls of every case as the emulation made them (gencalls.write_cases: sequences, the lists
    of every search and validation, the restatement's verdict per row, children and done[]) replayed by a program of its own under
    AddressSanitizer and UndefinedBehaviorSanitizer.  Nothing is loaded into python under a sanitizer"""
    cases = str(tmp_path / "cases.txt")
    G.write_cases(cases, [run(lib, case) for case in G.CASES])
    exe = str(tmp_path / "gen_calls_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPM_WAVE_EVENTS=5",
                    os.path.join(ROOT, "tests", "emu", "gen_calls_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, cases], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "gen_calls_check ok: %d cases" % len(G.CASES) in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
