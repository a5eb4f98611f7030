"""The designed blocks of tests/gapedges.py on the CPU: the host restatement of the gap aligner (parsnp_amd/csrc/host/gapalign.cpp)
against the reference's recorded rows on every block; floors that turn red when the generator stops reaching a path; the generator's
constants against the kernel's source; and the LONG form of the device gap aligner itself, executed on the host by tests/emu/gap_emu.cpp
(gapalign_hip.hip compiled unchanged, a fiber per lane) under an ascending and a descending schedule of lanes and wavefronts: the
recorded rows, the exact decline predicate, and a sentinel fill of out_rows that only the aligned jobs' rows may touch.  The
one-wavefront forms (narrow, wide, tall) run on the device only: tests/test_gpu_gap_edges.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gapedges
from test_gapalign import aligner  # noqa: F401  (fixture: the host restatement)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "parsnp_amd", "csrc", "engine", "gapalign_hip.hip")
PLAN = os.path.join(ROOT, "parsnp_amd", "csrc", "engine", "gap_plan.h")      # the forms' limits, included by the kernel's source
EMU_SRC = os.path.join(ROOT, "tests", "emu", "gap_emu.cpp")
EMU_STUB = os.path.join(ROOT, "tests", "emu", "hipstub")
EMU_LIB = os.path.join(ROOT, "tests", "emu", "libgap_emu.so")
SENTINEL = 0xEE


class Stats(C.Structure):
    _fields_ = [("jobs_narrow", C.c_int64), ("jobs_wide", C.c_int64), ("declined", C.c_int64), ("ms_narrow", C.c_double), ("ms_wide", C.c_double)]


class TallStats(C.Structure):
    _fields_ = [("jobs_narrow", C.c_int64), ("jobs_wide", C.c_int64), ("jobs_tall", C.c_int64), ("declined", C.c_int64),
                ("ms_narrow", C.c_double), ("ms_wide", C.c_double), ("ms_tall", C.c_double)]


class LongStats(C.Structure):
    _fields_ = [("jobs_narrow", C.c_int64), ("jobs_wide", C.c_int64), ("jobs_long", C.c_int64), ("declined", C.c_int64),
                ("ms_narrow", C.c_double), ("ms_wide", C.c_double), ("ms_long", C.c_double)]


STATS = {"batch": None, "wide": Stats, "tall": TallStats, "long": LongStats}


def run_call(L, call):
    """one call of the entry point of a gapedges.Call on the library L, checked in full: the reference's rows and column count for
    every job the exact predicate takes, cols = -1 for every other, the sentinel bytes intact in the row area of every declined job,
    between the areas and behind the last one, and the statistics record as the numbers the predicate gives -> the statistics"""
    row_off, out_bytes, verdict = gapedges.lay_out(call)
    jobs = call.jobs
    nseq = np.array([len(j.block) for j in jobs], np.int32)
    flat = [s.encode() for j in jobs for s in j.block]
    off = np.zeros(len(flat) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in flat])
    chars = np.frombuffer(b"".join(flat) or b"\0", np.uint8).copy()
    maxc = np.array([j.max_cols for j in jobs], np.int32)
    ro = np.array(row_off, np.int64)
    total = int((nseq.astype(np.int64) * maxc).sum())
    assert out_bytes == total - call.short_by
    out = np.full(total + 64, SENTINEL, np.uint8)
    cols = np.full(len(jobs), -7, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    st = STATS[call.entry]() if STATS[call.entry] else None
    head = (C.c_int(-1), C.c_int64(len(jobs)), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32), p(ro, C.c_int64),
            p(out, C.c_uint8), C.c_int64(out_bytes), p(cols, C.c_int32))
    L.pm_gap_last_error.restype = C.c_char_p
    if call.entry == "batch":
        L.pm_gap_align_batch.restype = C.c_int
        rc = L.pm_gap_align_batch(*head)
    else:
        fn = getattr(L, "pm_gap_align_groups_" + call.entry)
        fn.restype = C.c_int
        ge = np.array([len(jobs)], np.int64)
        rc = fn(*head, C.c_int(1), p(ge, C.c_int64), None, None, C.byref(st))
    assert rc == 0, L.pm_gap_last_error()
    expect = dict(narrow=0, wide=0, tall=0, long=0, declined=0)
    for k, (j, (ok, why)) in enumerate(zip(jobs, verdict)):
        base, w, n = row_off[k], j.max_cols, len(j.block)
        area = out[base: base + n * w]
        if ok:
            want = j.rows
            assert cols[k] == len(want[0]), (k, j.why, int(cols[k]), len(want[0]))
            got = [area[i * w: i * w + len(want[0])].tobytes().decode() for i in range(n)]
            assert got == want, (k, j.why)
            form = gapedges.form_of(j.block)
            expect["wide" if form == "narrow" and len(want[0]) > 96 else form] += 1
        else:
            assert cols[k] == -1, (k, j.why, why, int(cols[k]))
            assert (area == SENTINEL).all(), "the row area of declined job %d (%s: %s) was written" % (k, j.why, why)
            expect["declined"] += 1
    assert (out[total:] == SENTINEL).all(), "bytes behind the last row were written"
    if st is not None:
        assert st.declined == expect["declined"] and st.jobs_narrow == expect["narrow"] and st.jobs_wide == expect["wide"], \
            (st.declined, st.jobs_narrow, st.jobs_wide, expect)
        if call.entry == "tall":
            assert st.jobs_tall == expect["tall"], (st.jobs_tall, expect)
        if call.entry == "long":
            assert st.jobs_long == expect["long"], (st.jobs_long, expect)
    return st, expect


def block_call(entry, topic, pick=None, slack=None):
    """the blocks of a topic as ONE call of an entry point: max_cols = the reference's column count + k % 3 (the capacity is tight),
    every job taken"""
    cs, rows = gapedges.cases(topic), gapedges.reference_rows(topic)
    jobs = [gapedges.Job(c.block, len(r[0]) + (k % 3 if slack is None else slack), r, c.name) for k, (c, r) in enumerate(zip(cs, rows)) if pick is None or pick(c)]
    assert jobs
    return gapedges.Call(entry, jobs, 0)


# ---- the restatement against the record

@pytest.mark.parametrize("topic", list(gapedges.TOPICS))
def test_restatement_equals_the_record(aligner, topic):  # noqa: F811
    """parsnp_amd/csrc/host/gapalign.cpp gives the reference's rows on every designed block: it is the oracle wherever a device test
    needs rows for a max_cols variant"""
    cs, wants = gapedges.cases(topic), gapedges.reference_rows(topic)
    assert len(cs) == len(wants)
    for c, want in zip(cs, wants):
        assert len(want) == len(c.block) and len({len(r) for r in want}) == 1 and [r.replace("-", "") for r in want] == c.block, c.name      # the reference aligned it
        assert aligner(c.block) == want, c.name


def test_sequence_0_is_profile_a(aligner):  # noqa: F811
    """the derivation in gapedges' docstring: two alignments of AACAAA and CCACAC score alike, and in either order of the block the
    string at index 0 gets the leading gap -- which string is profile A goes by its index, in the reference and in the restatement"""
    names = [c.name for c in gapedges.cases("narrow_pairs")]
    ab, ba = (gapedges.reference_rows("narrow_pairs")[names.index(n)] for n in ("narrow order ab", "narrow order ba"))
    assert ab == ["-AACAAA", "CCACAC-"] and ba == ["-CCACAC", "AACAAA-"]
    assert aligner(["AACAAA", "CCACAC"]) == ab and aligner(["CCACAC", "AACAAA"]) == ba


# ---- generator floors, on the reference's rows

def _lengths(topic, tag):
    return {tuple(len(s) for s in c.block) for c in gapedges.cases(topic) if c.name.startswith(tag) and len(c.block) == 2}


def _kinds(topic, la, lb):
    return {c.name.split()[-1] for c in gapedges.cases(topic) if [len(s) for s in c.block] == [la, lb]}


def test_floor_lengths():
    long_ = _lengths("long_pairs", "long ")
    for la in (1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 320, 321, 322, 512, 513, 1023, 1024):
        assert (la, 321) in long_ and (la, 386) in long_, la
    for lb in (1, 2, 64, 65, 66, 129, 130, 255, 256, 257, 258, 322, 1023, 1024):
        assert (321, lb) in long_ and (385, lb) in long_, lb
    assert {(1024, 1024), (1023, 1024), (1024, 1), (1, 1024)} <= long_
    assert all(max(p) > 320 for p in long_)
    assert {"copy", "unrelated", "repeatA", "repeatAC", "straddle0", "straddle1"} == _kinds("long_pairs", 1024, 1024) == _kinds("long_pairs", 321, 322)
    assert {"copy", "unrelated", "repeatA", "repeatAC"} == _kinds("long_pairs", 1, 1024)
    wide = _lengths("wide_pairs", "wide ")
    for x in (97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320):
        assert {(x, 97), (x, 320), (97, x), (320, x)} <= wide, x
    assert all(96 < max(p) <= 320 for p in wide)
    narrow = _lengths("narrow_pairs", "narrow ")
    assert {(a, b) for a in (1, 2, 63, 64, 65, 95, 96) for b in (1, 2, 63, 64, 65, 95, 96)} <= narrow and all(max(p) <= 96 for p in narrow)
    assert {"copy", "unrelated", "repeatA", "repeatAC", "straddle0"} == _kinds("narrow_pairs", 96, 96)


def test_floor_column_counts():
    cols = {len(r[0]) for r in gapedges.reference_rows("narrow_pairs")}
    assert {64, 65, 96, 97} <= cols
    chunks = {(len(r[0]) + 63) // 64 for r in gapedges.reference_rows("wide_pairs")}
    assert set(range(2, 11)) <= chunks      # the right-to-left re-spelling of the wide form: 2, 3, .. 10 chunks of 64 columns
    assert max(len(r[0]) for r in gapedges.reference_rows("long_pairs")) > 1100


def _deleted_rows(rows):
    """the runs of sequence-0 positions (0-based rows of profile A) that the alignment deletes: [(first, last)]"""
    out, i, run = [], 0, None
    for a, b in zip(rows[0], rows[1]):
        if a != "-":
            if b == "-":
                run = (run[0], i) if run else (i, i)
            elif run:
                out.append(run)
                run = None
            i += 1
    return out + ([run] if run else [])


def _inserted_cols(rows):
    return _deleted_rows(rows[::-1])


def test_floor_straddles():
    """a deletion run that starts at or before row 64 (1-based: the last row of a stripe) and ends after it, likewise 256 (the last
    row of a round) and 320, in a long and (64, 256) in a wide block; and an insertion run across column 256 in a long block whose
    profile B is longer than the ring"""
    for topic, edges in (("long_pairs", (64, 256, 320)), ("wide_pairs", (64, 256)), ("narrow_pairs", (64,))):
        cs, rows = gapedges.cases(topic), gapedges.reference_rows(topic)
        for edge in edges:
            hits = [c.name for c, r in zip(cs, rows) if c.name.endswith("straddle0")
                    and any(a + 1 <= edge < b + 1 and b - a >= 15 for a, b in _deleted_rows(r))]
            assert len(hits) >= (1 if topic == "narrow_pairs" else 5), (topic, edge, hits)
    cs, rows = gapedges.cases("long_pairs"), gapedges.reference_rows("long_pairs")
    hits = [c.name for c, r in zip(cs, rows) if c.name.endswith("straddle1") and any(a + 1 <= 256 < b + 1 and b - a >= 15 for a, b in _inserted_cols(r))]
    assert len(hits) >= 10, hits


def _multiplicity(s, mer):
    return sum(s[i:i + len(mer)] == mer for i in range(len(s) - len(mer) + 1))


def test_floor_counts_and_wildcards():
    for form in ("wide", "long"):
        cs = gapedges.cases("counts_" + form)
        for name in ("%s counts 255 256 257" % form, "%s counts beside short strings" % form):
            blk = next(c.block for c in cs if c.name == name)
            assert [_multiplicity(s, "AAAAAA") for s in blk[:3]] == [255, 256, 257], name
        assert {5, 6, 7} <= {len(s) for s in next(c.block for c in cs if c.name.endswith("beside short strings"))}
    for form in ("narrow", "wide", "long"):
        cs = gapedges.cases("counts_" + form)
        assert {1, 3, 5, 6, 7} <= {len(s) for s in next(c.block for c in cs if c.name == "%s short strings" % form)}
        blk = next(c.block for c in cs if c.name.endswith("N in every 6-mer"))
        assert all("N" in s[i:i + 6] for s in blk[:3] for i in range(len(s) - 5) if i + 6 <= 50)
        assert set(gapedges.WILD) <= set("".join(next(c.block for c in cs if c.name.endswith("wildcards"))))
        assert all(gapedges.form_of(c.block) == form for c in cs), form


def test_floor_distinct_and_ties():
    for form in ("narrow", "wide", "long"):
        cs = {c.name[len(form) + 1:]: c.block for c in gapedges.cases("distinct_" + form)}
        assert all(gapedges.form_of(b) == form for b in cs.values())
        for n, firsts in ((130, (0, 63, 64, 65, 127, 128, 129)), (257, (0, 63, 64, 65, 127, 128, 129, 255, 256))):
            blk = cs["firsts %d" % n]
            assert len(blk) == n and tuple(i for i, s in enumerate(blk) if s not in blk[:i]) == firsts
        assert len(set(cs["all identical"])) == 1 and len(cs["all identical"]) >= 3
        assert cs["s t s t"][0::2] == [cs["s t s t"][0]] * 4 and cs["s t s t"][1::2] == [cs["s t s t"][1]] * 4 and cs["s t s t"][0] != cs["s t s t"][1]
        blk = cs["zero pairs 5-70 64-129"]
        assert [(i, j) for j in range(len(blk)) for i in range(j) if blk[i] == blk[j]] == [(5, 70), (64, 129)]
        assert [len(cs["count %d" % n]) for n in (2, 3, 63, 64, 65, 128, 129, 255, 256, 257, 512)] == [2, 3, 63, 64, 65, 128, 129, 255, 256, 257, 512]
    assert [len(c.block) for c in gapedges.cases("tall")] == [513, 576, 577, 2047, 2048, 513, 2048]
    assert all(1 <= len(s) <= 3 for c in gapedges.cases("tall")[:5] for s in c.block)
    last = gapedges.cases("tall")[6].block
    assert {len(s) for s in last} == {320} and len(set(last)) == 2
    assert len(gapedges.too_tall()) == 2049
    for c, n in zip(gapedges.cases("long_many"), (255, 256, 257)):
        assert len(c.block) == n and 321 <= len(c.block[0]) <= 400 and all(1 <= len(s) <= 12 for s in c.block[1:])


ALL_CALLS = [("narrow", 40), ("wide", 40), ("long", 40)]


def test_floor_decline_reasons():
    """at least one taken and one declined case of every decline reason, per entry point"""
    for form in ("narrow", "wide", "tall", "long"):
        calls = gapedges.capacity_calls(form)
        seen = set()
        for call in calls:
            _, _, verdict = gapedges.lay_out(call)
            seen |= {why for _, why in verdict}
            assert sum(ok for ok, _ in verdict) >= 3
        assert {None, "n", "alphabet", "cols", "out_bytes"} <= seen, (form, seen)
        if form != "tall":
            assert "len" in seen
        # the last job is taken with out_bytes exact and declined for out_bytes alone with one byte less
        assert gapedges.lay_out(calls[0])[2][-1] == (True, None) and gapedges.lay_out(calls[1])[2][-1] == (False, "out_bytes")
        assert gapedges.lay_out(calls[0])[2][:-1] == gapedges.lay_out(calls[1])[2][:-1]
        why = {j.why: v for j, v in zip(calls[0].jobs, gapedges.lay_out(calls[0])[2])}
        assert why["max_cols exact"] == (True, None) and why["max_cols one short"] == (False, "cols")
        j = next(j for j in calls[0].jobs if j.why == "a string longer than its own max_cols")
        assert j.max_cols < max(len(s) for s in j.block) <= max(min(x.max_cols, gapedges.LIMITS[form][2]) for x in calls[0].jobs if gapedges.form_of(x.block) == form)
    verdict = gapedges.lay_out(gapedges.second_wide_run()[0])[2]
    assert sum(ok for ok, _ in verdict) >= 5 and sum(why == "cols" for _, why in verdict) >= 3
    for form, count in ALL_CALLS:
        v = gapedges.lay_out(gapedges.slot_reuse(form, count))[2]
        assert [why for _, why in v][:11] == [None] * 6 + ["cols"] + [None] * 3 + ["alphabet"]


def test_generator_matches_the_kernel():
    """the constants the generator places its edges by, read out of the kernel's source"""
    src = open(PLAN).read() + open(KERNEL).read()
    got = {}
    for name in gapedges.CONSTANTS:
        m = re.search(r"\bconstexpr int (?:\w+ = \d+, )*%s = (\d+)" % name, src)
        assert m, name
        got[name] = int(m.group(1))
    assert got == gapedges.CONSTANTS
    assert gapedges.LIMITS == {"narrow": (got["kMaxSeqs"], got["kMaxCols"], got["kMaxCols"]), "wide": (got["kMaxSeqs"], got["kWideSeq"], got["kWideCols"]),
                               "tall": (got["kTallSeqs"], got["kWideSeq"], got["kWideCols"]), "long": (got["kLongSeqs"], got["kLongSeq"], got["kLongCols"])}
    # the places the edges come from: the stripe of 64 rows, the round of four wavefronts, the ring mask, the chunk count
    assert "for (int r0 = 0; r0 < la; r0 += 4 * 64)" in src and "const int s0 = r0 + wave * 64;" in src
    assert "const int chunks = (64 + lb - 1 + kLongChunk - 1) / kLongChunk;" in src and "const int rounds_chunks = chunks + 3 * kLongLag;" in src
    assert "in_mask = wave == 0 ? 4095 : kLongRing - 1, out_mask = wave == 3 ? 4095 : kLongRing - 1;" in src
    assert "if (first) em = (uint8_t)(cnt & 255);" in src and "const int c1 = lane, c2 = lane + 64;" in src
    assert got["kLongThreads"] == 4 * 64 and got["kLongChunk"] == 64 and 4 * got["kLongChunk"] == got["kLongRing"]
    # (the routing rule, now route() of gap_plan.h; tests/test_gap_plan.py runs it)
    assert "return n > kMaxSeqs ? (w > kWideSeq ? kLongTall : kTall) : (w > kWideSeq ? kLong : (w > kMaxCols ? kWide : kNarrow));" in src


# ---- the long form, executed on the host

@pytest.fixture(scope="module")
def emu_long():
    deps = [EMU_SRC, KERNEL, PLAN, os.path.join(EMU_STUB, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "parsnp_mum.h")]
    if not os.path.exists(EMU_LIB) or os.path.getmtime(EMU_LIB) < max(os.path.getmtime(d) for d in deps):
        tmp = EMU_LIB[:-len(".so")] + ".%d.so" % os.getpid()
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w", "-ffp-contract=off", "-I" + EMU_STUB, "-x", "c++", EMU_SRC, "-o", tmp], check=True)
        os.replace(tmp, EMU_LIB)
    assert "PM_GAP_EMU_REVERSE" not in os.environ and "PM_GAP_EMU_CUS" not in os.environ
    return C.CDLL(EMU_LIB)


SCHEDULES = pytest.mark.parametrize("descending", [0, 1], ids=["ascending", "descending"])
@SCHEDULES
def test_emulated_long_pairs(emu_long, descending):
    emu_long.gap_emu_set_schedule(descending)
    st, expect = run_call(emu_long, block_call("long", "long_pairs"))
    assert expect["long"] == len(gapedges.cases("long_pairs")) >= 380 and expect["declined"] == 0


@SCHEDULES
def test_emulated_long_counts_distinct_and_many(emu_long, descending):
    """the long multi-sequence blocks of up to 130 sequences, and the three of long_many: one long string beside 254, 255 and 256 short
    ones, all distinct -- the strides of the 256-thread loops and of the partner-per-wavefront loop.  The device alone runs
    "long firsts 257" and "long count 255 / 256 / 257 / 512" (1 536 pairwise steps: half a minute per schedule here)"""
    emu_long.gap_emu_set_schedule(descending)
    for topic in ("counts_long", "distinct_long", "long_many"):
        st, expect = run_call(emu_long, block_call("long", topic, pick=lambda c: topic != "distinct_long" or len(c.block) <= 130))
        assert expect["declined"] == 0 and expect["long"] == len(gapedges.cases(topic)) - 5 * (topic == "distinct_long")


@SCHEDULES
def test_emulated_long_capacity_and_declines(emu_long, descending):
    emu_long.gap_emu_set_schedule(descending)
    for call in gapedges.capacity_calls("long"):
        st, expect = run_call(emu_long, call)
        assert expect["long"] >= 3 and expect["declined"] >= 6


@SCHEDULES
def test_emulated_long_slot_reuse(emu_long, descending):
    """the emulation runs the workgroups of a launch one after the other, so its first slot takes every job of the list: 40 jobs, with
    the late and the early declines between the taken ones"""
    emu_long.gap_emu_set_schedule(descending)
    st, expect = run_call(emu_long, gapedges.slot_reuse("long", 40))
    assert expect["long"] == 40 - 5 - 3 and expect["declined"] == 8


def test_emulation_refuses_the_one_wavefront_forms(emu_long):
    """a call with a narrow or a wide job would launch gap_align_kernel (64 threads), whose lockstep the emulation does not have: error"""
    emu_long.gap_emu_set_schedule(0)
    nseq = np.array([2], np.int32); off = np.array([0, 4, 8], np.int64); chars = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    maxc = np.array([16], np.int32); row_off = np.zeros(1, np.int64); out = np.zeros(33, np.uint8); cols = np.full(1, -7, np.int32)
    ge = np.array([1], np.int64)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    emu_long.pm_gap_align_groups_long.restype = C.c_int
    rc = emu_long.pm_gap_align_groups_long(C.c_int(-1), C.c_int64(1), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32), p(row_off, C.c_int64),
                                           p(out, C.c_uint8), C.c_int64(33), p(cols, C.c_int32), C.c_int(1), p(ge, C.c_int64), None, None, None)
    assert rc != 0
