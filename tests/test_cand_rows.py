"""The candidate side of a search call (include/parsnp_mum.h: pm_multi_mum_batch) row by row against the sequential restatement of
tests/candrows.py, in the kernel emulation (tests/emu: one host thread plays every lane of CoarseFill, MasterEPSeg / MasterEP, CandMark,
CandWrite, FoldCandidates, OkCount, CompactSp, CompactCandidates, DirtyExtent, DirtyPrefix, DirtyMark and DirtyMerge through their
sequential `#else` bodies).  tests/test_gpu_cand_rows.py runs the same checks on the device, where the `__HIP_DEVICE_COMPILE__` bodies
and the grouped downloads (pm_copy_many) run.

1. the fold and Master.EP at the edges of the 64-genome groups, (k, lon, sp, fwd) exactly, "master_seg" 1 and 0;  2. Master.EP at the
edges of its 256-position chunks and with more events than its staging area holds;  3. the candidate listing of a batch of seven
regions, (sp, fwd) and MUM rows;  4. the MUM rows and the overlap flags of a long one-region list (rows to the host and resident), list
lengths around "dirty_min", rows per block, blocks per round, the deciding pair and genome, the four equalities, rows of 4 and 5
bases;  5. three anchor calls of one session whose capacities carry over;  6. the downloads with and without "copy_kernel".

A failure is reported as (case, tunes, first differing row, genome, want, got).  Every case asserts its floors from the restatement
alone (test_floors, which also pins the recorded numbers)."""
import os
import re
import subprocess

import pytest

import candrows as R
from parsnp_amd.binding import Lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 1 << 40      # a "dirty_min" no list reaches
SEGS = ({"master_seg": 1}, {"master_seg": 0})
CHUNK_CASES = [(s, t, late) for s in R.CHUNK_STARTS for t in R.CHUNK_TAILS for late in (False, True)]
DOWNLOAD_CASES = ("g65_257", "g65_300", "rows4097")
COUNTS = (0, 6, 7, 8)      # substitutions of the one query: 1, 7, 8 and 9 candidates before the fold (around the eight XCDs of xcd_item)


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


_want = {}


def expect(key, seqs, starts, lens, minsize, dirty_min, rows=True):
    """the restatement of one call, once per process"""
    key = (key, tuple(int(x) for x in minsize), dirty_min, rows)
    if key not in _want:
        _want[key] = R.Expect(seqs, starts, lens, minsize, dirty_min, rows)
    return _want[key]


def call(lib, name, seqs, mode, tune, starts, lens, minsize, want):
    with R.RowSession(lib, seqs, mode, tune) as s:
        got = s.call(starts, lens, minsize)
    diff = R.compare(name, got, want, mode)
    assert diff is None, "(case, tunes, first differing row, genome, want, got) = %s" % ((diff[0], dict(tune or {}, rows=mode)) + diff[1:],)
    return got


def flag_want(name, dirty_min=8):
    seqs, ms = R.flag_case(name)
    st, ln = R.whole(seqs)
    return seqs, st, ln, [ms], expect(("flag", name), seqs, st, ln, [ms], dirty_min)


def short_want():
    seqs, ms = R.short_rows_set(R.SHORT_ROWS_SEED)
    st, ln = R.whole(seqs)
    return seqs, st, ln, [ms], expect("short_rows", seqs, st, ln, [ms], 2)


# ------------------------------------------------------------------------------------------------------------------ the floors
# what test_floors printed when the cases were written (the README row quotes them): per fold set (candidates before the fold,
# accepted, same-group clips, clips from the group before)
FOLD_RECORDED = {1: (4, 4, 0, 0), 63: (10, 9, 2, 0), 64: (14, 13, 3, 0), 65: (18, 17, 1, 3), 127: (26, 24, 3, 4), 128: (26, 24, 3, 4),
                 129: (28, 26, 1, 7), 193: (30, 28, 1, 8)}


def check_fold_floors(nq):
    seqs = R.fold_set(nq)
    assert 600 <= len(seqs[0]) <= 700, len(seqs[0])
    assert len(seqs[0]) % 4, "the reference's length is a multiple of 4"
    f = R.fold_floors(seqs, R.FOLD_MINSIZE)
    print("fold %d: %s" % (nq, f))
    last = nq - 1
    for p in (0, 62, 63, 64, 65, 127, 128, last):
        assert p >= nq or p in f["shortest"], "no candidate whose shortest reach is query %d's alone: %s" % (p, f)
    for t in (63, 64):
        assert t >= nq or t in f["ties"], "no tie of the two strands at query %d: %s" % (t, f)
    if nq > 10:
        assert f["clipped_same"] >= 1, f
    if nq > 70:
        assert f["clipped_before"] >= 1, f
    if nq > 1:
        assert f["listed"] > f["accepted"] and last in f["up_alone"], "no candidate that UP >= EP alone rejects through the last query: %s" % f
    if nq > 64:
        assert 64 in f["up_alone"], f
    assert (f["listed"], f["accepted"], f["clipped_same"], f["clipped_before"]) == FOLD_RECORDED[nq], (nq, f)


def check_count_floors():
    for subs in COUNTS:
        seqs = R.count_set(subs)
        st, ln = R.whole(seqs)
        m = R.region_mums(seqs, st[0], ln[0], R.FOLD_MINSIZE, want_master=True)
        assert len(R.listed_candidates(m[5], R.FOLD_MINSIZE)) == subs + 1 == len(m[0])


def check_chunk_floors(starts, tail, late):
    seqs = R.chunk_set(starts, tail, late)
    assert len(seqs[0]) == 3 * R.CHUNK + tail
    ev = R.events_of(seqs, R.CHUNK_MINSIZE)
    st, ln = R.whole(seqs)
    want = expect(("chunk", starts, tail, late), seqs, st, ln, [R.CHUNK_MINSIZE], NEVER, rows=False)
    for s in starts:
        assert all(s in ev[g] for g in (0, 2, 3)), "no event starts on reference position %d" % s
        assert s in want.k or (late and s < 300), "the event at %d makes no candidate" % s      # (the late query has nothing before 300)
    assert ev[1] and not [l for l in ev[1] if l >= R.CHUNK] and max(ev[1]) > 0, "query 1 has an event in the middle chunk or the last: %s" % ev[1]
    if late:
        assert ev[4] and min(ev[4]) >= R.CHUNK, "the late query has an event before the second chunk"
        assert want.k and min(want.k) >= R.CHUNK, "a candidate where one query's carry-in is 0"
        assert any(2 * R.CHUNK <= k for k in want.k) and any(k < 2 * R.CHUNK for k in want.k)
    else:
        assert all(any(c * R.CHUNK <= k < (c + 1) * R.CHUNK for k in want.k) for c in range(3)), want.k


def staging_totals():
    seqs = R.staging_set()
    ev = R.events_of(seqs, R.STAGE_MINSIZE)
    per = [[sum(1 for l in e if c * R.CHUNK <= l < (c + 1) * R.CHUNK) for c in range(3)] for e in ev]
    return [sum(p[c] for p in per[:R.LANES]) for c in range(3)], [sum(p[c] for p in per[R.LANES:]) for c in range(3)]


def check_staging_floors():
    first, second = staging_totals()
    print("staging: events per chunk of the first 64 queries %s, of the other 6 %s" % (first, second))
    assert first[1] > R.STAGE_CAP and max(second) <= R.STAGE_CAP and min(second) > 0, (first, second)


def check_batch_floors():
    seqs, st, ln, ms = R.batch_set()
    want = expect("batch", seqs, st, ln, ms, NEVER)
    flat, with_c, follows, reverse = R.batch_floors(want, ln)
    print("batch: flat positions mod 64 %s, candidates per region %s" % (sorted(flat), [want.off[r + 1] - want.off[r] for r in range(7)]))
    assert {63, 0, 1} <= flat, flat
    assert with_c == [True, True, True, False, True, False, True], with_c
    assert ln[3].max() == 0 and follows >= 1 and reverse == want.total >= 6
    assert all(x > 0 for x in st.ravel()), "a window starts at 0"
    assert not any(f & (R.ROW_BAD | R.ROW_OUTSIDE) for f in want.flags)


FLAG_FLOORS = {      # name -> floors on candrows.flag_floors (>=, or == for a list / the exact row count)
    "short40": dict(rows=40, a_eq_maxend_clean=1, early_only=1, early_dirty=2, clean_beside=3, a_eq_maxend=2, a_eq_maxend_m1=2, b_eq_minstart=1, pair_at_round_end=1, pair_inside_block=1),
    "rows255": dict(rows=255, a_eq_maxend_clean=2, early_dirty=3, clean_beside=2, a_eq_maxend_m1=2, b_eq_minstart_p1=1, pair_at_round_end=1, last_round_rows=7, flagged_in_last_round=2),
    "rows256": dict(rows=256, a_eq_maxend_clean=2, early_only=1, early_dirty=2, clean_beside=2, a_eq_maxend_m1=2, b_eq_minstart=1, pair_at_round_end=1, flagged_in_last_round=2),
    "rows257": dict(rows=257, a_eq_maxend_clean=2, early_only=1, early_dirty=3, a_eq_maxend_m1=2, pair_across_blocks=1, last_round_rows=1, flagged_in_last_round=1),
    "rows260": dict(rows=260, a_eq_maxend_clean=2, early_only=1, early_dirty=3, a_eq_maxend_m1=2, pair_across_blocks=1, last_round_rows=4, flagged_in_last_round=4),
    "rows512": dict(rows=512, a_eq_maxend_clean=2, early_only=1, early_dirty=2, b_eq_minstart=1, pair_across_blocks=1, decided_blocks_away=1),
    "rows513": dict(rows=513, a_eq_maxend_clean=2, early_dirty=3, b_eq_minstart_p1=1, pair_across_blocks=1, decided_blocks_away=2, last_round_rows=1, flagged_in_last_round=1),
    "rows4096": dict(rows=4096, a_eq_maxend_clean=2, early_only=1, early_dirty=3, b_eq_minstart=1, pair_across_blocks=1, pair_at_round_end=1, decided_blocks_away=15),
    "rows4097": dict(rows=4097, a_eq_maxend_clean=2, early_dirty=3, b_eq_minstart_p1=1, pair_across_blocks=1, decided_blocks_away=16, last_round_rows=1, flagged_in_last_round=1),
    "g65_257": dict(rows=257, a_eq_maxend_clean=2, early_only=1, early_dirty=3, deciding_columns=[1, 63, 64], past_first_group_only=1, b_eq_minstart=1, strand_bytes=257 * 65),
    "g65_300": dict(rows=300, a_eq_maxend_clean=2, early_dirty=4, deciding_columns=[1, 2, 63, 64], past_first_group_only=1, early_here_dirty_there=1, start_bytes=4 * 300 * 65),
    "g130_300": dict(rows=300, a_eq_maxend_clean=2, early_dirty=7, deciding_columns=[1, 2, 63, 64, 65, 70, 128, 129], past_first_group_only=3, early_here_dirty_there=1),
}


def check_flag_floors(name):
    seqs, st, ln, ms, want = flag_want(name)
    f = R.flag_floors(name, want)
    print("%s: %s" % (name, f))
    assert want.long_list and not any(x & (R.ROW_BAD | R.ROW_OUTSIDE) for x in want.flags)
    for k, v in FLAG_FLOORS[name].items():
        assert (f[k] == v) if k in ("rows", "deciding_columns", "strand_bytes", "start_bytes", "last_round_rows") else (f[k] >= v), "%s: %s = %s, the floor is %s" % (name, k, f[k], v)
    if name in DOWNLOAD_CASES:
        assert name != "g65_257" or f["strand_bytes"] % 4, "no download whose byte count is no multiple of 4"
        assert name == "g65_257" or f["start_bytes"] > R.COPY_PIECE, "no download of more than one piece"


def check_short_floors():
    seqs, st, ln, ms, want = short_want()
    four, five, moved, kept = R.short_rows_floors(want)
    print("short rows: %d of 4 bases, %d of 5, %d rows that rows of 4 would flag otherwise, %d that need the rows of 5" % (four, five, moved, kept))
    assert want.long_list and min(four, five, moved, kept) >= 1


def capacity_counts():
    seqs = R.capacity_set()
    st, ln = R.whole(seqs)
    return [len(R.listed_candidates(R.region_mums(seqs, st[0], ln[0], ms, want_master=True)[5], ms)) for ms in R.CAP_MINSIZE]


def check_capacity_floors():
    x, y, z = capacity_counts()
    print("capacities: %d, %d and %d candidates before the fold" % (x, y, z))
    assert y <= x + x // 8 + 256 and 8 * z > 9 * x + 8 * 256 and x >= 8, (x, y, z)      # (z > 1.125 x + 256)


# ------------------------------------------------------------------------------------------------------------------ the checks
def check_fold(lib, nq):
    seqs = R.fold_set(nq)
    st, ln = R.whole(seqs)
    want = expect(("fold", nq), seqs, st, ln, [R.FOLD_MINSIZE], NEVER, rows=False)
    return [call(lib, "fold %d" % nq, seqs, 0, tune, st, ln, [R.FOLD_MINSIZE], want) for tune in SEGS]


def check_counts(lib):
    for subs in COUNTS:
        seqs = R.count_set(subs)
        st, ln = R.whole(seqs)
        want = expect(("count", subs), seqs, st, ln, [R.FOLD_MINSIZE], NEVER, rows=False)
        for tune in SEGS:
            got = call(lib, "count %d" % subs, seqs, 0, tune, st, ln, [R.FOLD_MINSIZE], want)
            assert int(got.timing["n_candidates"]) == subs + 1 == int(got.timing["n_accepted"]), (subs, got.timing)      # (the engine's own counts)


def check_chunks(lib, starts, tail, late):
    seqs = R.chunk_set(starts, tail, late)
    st, ln = R.whole(seqs)
    want = expect(("chunk", starts, tail, late), seqs, st, ln, [R.CHUNK_MINSIZE], NEVER, rows=False)
    for tune in SEGS:
        call(lib, "chunk %s + %d%s" % (starts, tail, " late" if late else ""), seqs, 0, tune, st, ln, [R.CHUNK_MINSIZE], want)


def check_staging(lib):
    seqs = R.staging_set()
    st, ln = R.whole(seqs)
    want = expect("staging", seqs, st, ln, [R.STAGE_MINSIZE], NEVER, rows=False)
    for tune in SEGS:
        call(lib, "staging", seqs, 0, tune, st, ln, [R.STAGE_MINSIZE], want)


def check_batch(lib):
    seqs, st, ln, ms = R.batch_set()
    want = expect("batch", seqs, st, ln, ms, NEVER)
    for mode in (0, 1):
        for tune in SEGS:
            call(lib, "batch", seqs, mode, tune, st, ln, ms, want)


def check_flags(lib, name, mode):
    seqs, st, ln, ms, want = flag_want(name)
    return call(lib, name, seqs, mode, {"dirty_min": 8}, st, ln, ms, want)


def check_list_lengths(lib, name="short40"):
    """a list of exactly dirty_min - 1, dirty_min and dirty_min + 1 rows: below dirty_min no bit, no table, dirty_known 0"""
    rows = FLAG_FLOORS[name]["rows"]
    for dirty_min in (rows + 1, rows, rows - 1):
        seqs, st, ln, ms, want = flag_want(name, dirty_min)
        assert want.long_list == (dirty_min <= rows) and (want.long_list or not any(f & (R.ROW_EARLY | R.ROW_DIRTY) for f in want.flags))
        for mode in (1, 2):
            call(lib, name, seqs, mode, {"dirty_min": dirty_min}, st, ln, ms, want)


def check_short_rows(lib):
    seqs, st, ln, ms, want = short_want()
    for mode in (1, 2):
        call(lib, "short rows", seqs, mode, {"dirty_min": 2}, st, ln, ms, want)


def check_capacities(lib):
    """three anchor calls of one resident session: the second sizes its tail from the first and fits, the third holds more candidates
    than the capacity it takes from the second and repeats its tail; with "fast_tail" = 0 no call repeats anything; the same rows"""
    seqs = R.capacity_set()
    st, ln = R.whole(seqs)
    out = []
    for fast in (1, 0):
        tune = {"dirty_min": 8, "fast_tail": fast}
        with R.RowSession(lib, seqs, 2, tune) as s:
            for i, ms in enumerate(R.CAP_MINSIZE):
                want = expect("cap", seqs, st, ln, [ms], 8)
                got = s.call(st, ln, [ms])
                diff = R.compare("capacities, call %d" % (i + 1), got, want, 2)
                assert diff is None, "(case, tunes, first differing row, genome, want, got) = %s" % ((diff[0], tune) + diff[1:],)
                repeats = got.timing.get("tail_repeats", 0)
                assert (repeats >= 1) if (fast and i == 2) else ("tail_repeats" not in got.timing), (fast, i, got.timing)
                out.append((got.start.tobytes(), got.strand.tobytes(), got.flags.tobytes()))
    return out


def check_downloads(lib, name):
    """the rows and flags with every download a copy command of its own: identical bytes"""
    seqs, st, ln, ms, want = flag_want(name)
    a = call(lib, name, seqs, 1, {"dirty_min": 8}, st, ln, ms, want)
    b = call(lib, name, seqs, 1, {"dirty_min": 8, "copy_kernel": 0}, st, ln, ms, want)
    for x in ("off", "k", "lon", "start", "strand", "flags"):
        assert getattr(a, x).tobytes() == getattr(b, x).tobytes(), (name, x)


def every_case():
    """(name, seqs, mode, tune, [(starts, lens, minsize, Expect, tail)]) of every call the module makes: what the sanitized program replays"""
    for nq in R.FOLD_QUERIES:
        seqs = R.fold_set(nq)
        st, ln = R.whole(seqs)
        for tune in SEGS:
            yield "fold%d" % nq, seqs, 0, tune, [(st, ln, [R.FOLD_MINSIZE], expect(("fold", nq), seqs, st, ln, [R.FOLD_MINSIZE], NEVER, rows=False), -1)]
    for subs in COUNTS:
        seqs = R.count_set(subs)
        st, ln = R.whole(seqs)
        yield "count%d" % subs, seqs, 0, {}, [(st, ln, [R.FOLD_MINSIZE], expect(("count", subs), seqs, st, ln, [R.FOLD_MINSIZE], NEVER, rows=False), -1)]
    for starts, tail, late in CHUNK_CASES:
        seqs = R.chunk_set(starts, tail, late)
        st, ln = R.whole(seqs)
        for tune in SEGS:
            yield "chunk", seqs, 0, tune, [(st, ln, [R.CHUNK_MINSIZE], expect(("chunk", starts, tail, late), seqs, st, ln, [R.CHUNK_MINSIZE], NEVER, rows=False), -1)]
    seqs = R.staging_set()
    st, ln = R.whole(seqs)
    yield "staging", seqs, 0, SEGS[1], [(st, ln, [R.STAGE_MINSIZE], expect("staging", seqs, st, ln, [R.STAGE_MINSIZE], NEVER, rows=False), -1)]
    seqs, st, ln, ms = R.batch_set()
    for mode in (0, 1):
        yield "batch", seqs, mode, {}, [(st, ln, ms, expect("batch", seqs, st, ln, ms, NEVER), -1)]
    for name in R.FLAG_CASES:
        seqs, st, ln, ms, want = flag_want(name)
        for mode in (1, 2):
            yield name, seqs, mode, {"dirty_min": 8}, [(st, ln, ms, want, -1)]
    for dirty_min in (41, 40, 39):
        seqs, st, ln, ms, want = flag_want("short40", dirty_min)
        yield "short40_%d" % dirty_min, seqs, 2, {"dirty_min": dirty_min}, [(st, ln, ms, want, -1)]
    seqs, st, ln, ms, want = short_want()
    yield "short_rows", seqs, 1, {"dirty_min": 2}, [(st, ln, ms, want, -1)]
    seqs = R.capacity_set()
    st, ln = R.whole(seqs)
    for fast in (1, 0):
        yield "capacities", seqs, 2, {"dirty_min": 8, "fast_tail": fast}, [(st, ln, [ms], expect("cap", seqs, st, ln, [ms], 8), 1 if fast and i == 2 else 0)
                                                                           for i, ms in enumerate(R.CAP_MINSIZE)]


# ------------------------------------------------------------------------------------------------------------------ the tests
FAMILIES = ["fold%d" % nq for nq in R.FOLD_QUERIES] + ["counts", "chunks", "staging", "batch"] + list(R.FLAG_CASES) + ["short_rows", "capacities"]


def check_floors(family):
    if family.startswith("fold"):
        check_fold_floors(int(family[4:]))
    elif family == "counts":
        check_count_floors()
    elif family == "chunks":
        for c in CHUNK_CASES:
            check_chunk_floors(*c)
    elif family == "staging":
        check_staging_floors()
    elif family == "batch":
        check_batch_floors()
    elif family == "short_rows":
        check_short_floors()
    elif family == "capacities":
        check_capacity_floors()
    else:
        check_flag_floors(family)


@pytest.mark.parametrize("family", FAMILIES)
def test_floors(cpu_checkers, family):
    """on the restatement alone: the engine is not loaded"""
    check_floors(family)


@pytest.mark.parametrize("nq", R.FOLD_QUERIES)
def test_fold_at_group_edges(lib, nq):
    check_fold(lib, nq)


def test_candidate_counts(lib):
    check_counts(lib)


@pytest.mark.parametrize("starts,tail,late", CHUNK_CASES)
def test_chunk_edges(lib, starts, tail, late):
    check_chunks(lib, starts, tail, late)


def test_staging_overflow(lib):
    check_staging(lib)


def test_batch_listing(lib):
    check_batch(lib)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(R.FLAG_CASES))
def test_overlap_flags(lib, name, mode):
    check_flags(lib, name, mode)


def test_list_lengths_around_dirty_min(lib):
    check_list_lengths(lib)


def test_rows_of_four_and_five_bases(lib):
    check_short_rows(lib)


def test_capacities_carried_over(lib):
    check_capacities(lib)


@pytest.mark.parametrize("name", DOWNLOAD_CASES)
def test_downloads(lib, name):
    check_downloads(lib, name)


def test_generator_matches_the_source():
    """the constants candrows.py restates, and how `posbase` lays the regions of a batch out, as the sources have them"""
    eng = os.path.join(ROOT, "parsnp_amd", "csrc", "engine")
    kernels = open(os.path.join(eng, "kernels.h")).read()
    core = open(os.path.join(eng, "engine_core.h")).read()
    hip = open(os.path.join(eng, "engine_hip.hip")).read()
    header = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    assert int(re.search(r"constexpr int kDirtyBlock = (\d+);", kernels).group(1)) == R.DIRTY_BLOCK
    assert int(re.search(r"constexpr int kEpCap = (\d+);", kernels).group(1)) == R.STAGE_CAP
    assert int(re.search(r"constexpr int kCoarseShift = (\d+);", kernels).group(1)) == 8 and R.CHUNK == 256
    assert re.search(r"for \(int64_t cb = c0; cb < c1; cb \+= (\d+)\)", kernels).group(1) == str(R.MARK_ROUND)
    assert re.search(r"for \(int64_t b0 = 0; b0 < nblocks; b0 \+= (\d+)\)", kernels).group(1) == str(R.PREFIX_ROUND)
    # the regions' reference windows one behind the other, in request order: flat position = sum of the earlier windows + l
    assert "ri.posbase = npos; posbase[(size_t)r] = npos; npos += ri.nR;" in core
    assert "(uint64_t)(hint.ncand + hint.ncand / 8 + 256)" in core      # the capacity check_capacity_floors restates
    assert "blockIdx.x - jobs.first_block[j]) << 16" in hip and R.COPY_PIECE == 1 << 16
    bits = {k: int(v) for k, v in re.findall(r"#define (PM_ROW_[A-Z]+) (\d+)u", header)}
    assert [bits["PM_ROW_" + x] for x in ("BAD", "OUTSIDE", "REVERSE", "DIRTY", "EARLY")] == [R.ROW_BAD, R.ROW_OUTSIDE, R.ROW_REVERSE, R.ROW_DIRTY, R.ROW_EARLY]
    assert int(re.search(r"int64_t dirty_min = (\d+);", core).group(1)) == 4096


def test_sanitized_program(lib, tmp_path):
    """tests/emu/cand_rows_check.cpp: the calls of every case, with the restatement's rows, replayed by a program of its own under
    AddressSanitizer and UndefinedBehaviorSanitizer.  Nothing is loaded into python under a sanitizer"""
    cases = str(tmp_path / "cases.txt")
    n = 0
    with open(cases, "w") as f:
        for name, seqs, mode, tune, calls in every_case():
            R.write_case(f, name, seqs, mode, tune, calls)
            n += 1
    exe = str(tmp_path / "cand_rows_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPM_WAVE_EVENTS=5",
                    os.path.join(ROOT, "tests", "emu", "cand_rows_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, cases], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "cand_rows_check ok: %d cases" % n in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
