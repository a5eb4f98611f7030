"""The long form of the device gap aligner (pm_gap_align_groups_long, include/parsnp_mum.h): gaps of up to 512 sequences of up to
1 024 bases and 2 048 columns, one workgroup of four wavefronts per gap -- what a cluster distance d of up to 1 000 produces.  The
bar is the reference's rows (libMUSCLE through oracle/_ref/muscle_ref, recorded in tests/golden/muscle_long_runs.json.xz and
gapalign.json) and the reference binary's whole runs at d = 1000 (tests/golden/long_gap_runs.json.xz); a job is declined
(cols = -1) exactly when it lies outside pm_gap_limits_long, and no job of the long family is."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gapgen
import longgen
import widegen
from parsnp_amd.paths import HIP_LIB
from test_gpu_tall_gaps import TallStats
from test_gpu_tall_gaps import align as align_tall
from test_gpu_wide_gaps import Stats, capacity, inside
from test_gpu_wide_gaps import align as align_wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LongStats(C.Structure):
    _fields_ = [("jobs_narrow", C.c_int64), ("jobs_wide", C.c_int64), ("jobs_long", C.c_int64), ("declined", C.c_int64),
                ("ms_narrow", C.c_double), ("ms_wide", C.c_double), ("ms_long", C.c_double)]


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(HIP_LIB)
    L.pm_gap_align_batch.restype = C.c_int
    L.pm_gap_align_groups_wide.restype = C.c_int
    L.pm_gap_align_groups_tall.restype = C.c_int
    L.pm_gap_last_error.restype = C.c_char_p
    assert hasattr(L, "pm_gap_align_groups_long") and hasattr(L, "pm_gap_limits_long"), "this library has no long form of the gap aligner"
    L.pm_gap_align_groups_long.restype = C.c_int
    return L


def limits_long(L):
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    assert L.pm_gap_limits_long(C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


def align(L, blocks, maxc, group_end=None, on_group=None):
    """pm_gap_align_groups_long -> (per block: list of rows, or None where the device declined; the call's statistics)"""
    nseq = np.array([len(b) for b in blocks], np.int32)
    flat = [s.encode() for b in blocks for s in b]
    off = np.zeros(len(flat) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in flat])
    chars = np.frombuffer(b"".join(flat) or b"\0", np.uint8).copy()
    maxc = np.array(maxc, np.int32)
    row_off = np.zeros(len(blocks), np.int64)
    row_off[1:] = np.cumsum(nseq[:-1].astype(np.int64) * maxc[:-1])
    out = np.zeros(int((nseq.astype(np.int64) * maxc).sum()) + 1, np.uint8)
    cols = np.full(len(blocks), -7, np.int32)
    group_end = np.array([len(blocks)] if group_end is None else group_end, np.int64)
    st = LongStats()

    def rows_of(j):
        if cols[j] < 0:
            return None
        base, w = int(row_off[j]), int(maxc[j])
        return [out[base + i * w: base + i * w + int(cols[j])].tobytes().decode() for i in range(len(blocks[j]))]

    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
    cb = CB(lambda ctx, g: on_group(g, [rows_of(j) for j in range(0 if g == 0 else int(group_end[g - 1]), int(group_end[g]))]) if on_group else None)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    rc = L.pm_gap_align_groups_long(C.c_int(-1), C.c_int64(len(blocks)), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32),
                                    p(row_off, C.c_int64), p(out, C.c_uint8), C.c_int64(len(out)), p(cols, C.c_int32), C.c_int(len(group_end)),
                                    p(group_end, C.c_int64), cb, None, C.byref(st))
    assert rc == 0, L.pm_gap_last_error()
    assert all(c == -1 or c >= 1 for c in cols)
    return [rows_of(j) for j in range(len(blocks))], st


def test_limits_are_the_documented_ones(lib):
    assert limits_long(lib) == (longgen.LONG_SEQS, longgen.LONG_SEQ_LEN, longgen.LONG_COLS) == (512, 1024, 2048)


def test_long_blocks_and_committed_vectors_against_the_reference(lib):
    """the long family and every committed vector of the narrow tests in ONE call: the reference's rows for every block inside the long
    limits, cols = -1 exactly for those outside; none of the long family is declined, and all of it runs in the long form"""
    lim = limits_long(lib)
    family = longgen.long_blocks()
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "gapalign.json")))
    blocks = family + [b["in"] for b in data]
    wants = longgen.reference_align(family) + [b["out"] for b in data]
    got, st = align(lib, blocks, [capacity(b, lim[2]) for b in blocks])
    declined = 0
    for k, (blk, want, rows) in enumerate(zip(blocks, wants, got)):
        if inside(blk, want, lim) and len(want[0]) <= capacity(blk, lim[2]):
            assert rows == want, (k, len(blk), blk[0][:40])
        else:
            assert rows is None, (k, len(blk), blk[0][:40])
            declined += 1
            assert k >= len(family), "a block of the long family was declined"
    assert all(r is not None for r in got[:len(family)])
    assert st.declined == declined and st.jobs_narrow + st.jobs_wide + st.jobs_long + st.declined == len(blocks)
    assert st.jobs_long >= len(family) and st.jobs_narrow > 200 and st.ms_long > 0


def test_mixed_groups_match_single_jobs(lib):
    """narrow, wide and long jobs interleaved in one call, in five groups with a `done` callback -- one group of long jobs only, one
    holding only a job with a 1 025-base string and a 513-sequence job (both declined): the rows of one job per call, every group
    reported in order with its rows in place"""
    lim = limits_long(lib)
    long_ = [b for b in longgen.long_blocks() if len(b) <= 50]
    wide = [b for b in widegen.wide_blocks() if len(b) <= 50]
    narrow = gapgen.blocks(79, 30, lengths=(2, 5, 13, 30, 60, 90))
    too_long = ["A" * (lim[1] + 1), "ACGT"]
    too_many = [long_[0][0]] * (lim[0] + 1)
    assert len(long_) >= 10 and len(wide) >= 8
    blocks = narrow[:10] + [long_[0]] + wide[:3] + [long_[1]] + narrow[10:20] + long_[2:6] + [too_long, too_many] + wide[3:6] + [long_[6]] + narrow[20:] + long_[7:10]
    group_end = [15, 25, 29, 31, len(blocks)]
    maxc = [capacity(b, lim[2]) for b in blocks]
    single = [align(lib, [b], [c])[0][0] for b, c in zip(blocks, maxc)]
    assert all(s is None for s in single[29:31]) and sum(s is None for s in single) == 2
    seen = []
    got, st = align(lib, blocks, maxc, group_end=group_end,
                    on_group=lambda g, rows: seen.append((g, rows == single[(0 if g == 0 else group_end[g - 1]):group_end[g]])))
    assert seen == [(g, True) for g in range(5)]
    assert got == single
    assert st.declined == 2 and st.jobs_long == 10 and st.jobs_wide >= 6 and st.jobs_narrow + st.jobs_wide == 36
    assert st.ms_long > 0 and st.ms_wide > 0 and st.ms_narrow > 0


def test_older_entry_points_keep_their_limits(lib):
    """the 2 x 321 block comes back -1 from pm_gap_align_groups_wide and pm_gap_align_groups_tall, beside a job they take"""
    blk = longgen.long_blocks()[0]
    assert [len(s) for s in blk] == [widegen.WIDE_SEQ_LEN + 1] * 2
    small = [blk[0][:300], blk[1][:280]]
    got, st = align_wide(lib, [blk, small], [700, 640], entry="wide")
    assert got[0] is None and got[1] is not None
    assert isinstance(st, Stats) and st.declined == 1 and st.jobs_wide == 1
    got, st = align_tall(lib, [blk, small], [700, 640])
    assert got[0] is None and got[1] is not None
    assert isinstance(st, TallStats) and st.declined == 1 and st.jobs_wide == 1 and st.jobs_tall == 0


def test_long_windows_whole_run_on_device(tmp_path):
    """parsnp_core as shipped at d = 1000, 8 threads, on the set of tests/test_long_gaps.py: the reference binary's XMFA bytes and log
    counters, and no gap is aligned on the host -- the windows go to the long form"""
    from parsnp_amd.paths import CORE_BIN
    got, t = longgen.long_run(CORE_BIN, "long10x300k", tmp_path)
    assert t["gap_host"] == 0 and t["gap_device_narrow"] + t["gap_device_wide"] + t["gap_device_long"] == t["gap_jobs"], t
    assert t["gap_device_long"] >= 40 and t["gap_jobs_long"] >= 40 and t["gap_longest"] >= 800, t


def test_two_hundred_genomes_with_long_windows(tmp_path):
    """200 genomes of 150 kb with 30 windows of 24 haplotypes the same way, 16 threads: every gap has 201 sequences"""
    from parsnp_amd.paths import CORE_BIN
    got, t = longgen.long_run(CORE_BIN, "long200x150k", tmp_path, threads=16)
    assert t["gap_host"] == 0 and t["gap_device_narrow"] + t["gap_device_wide"] + t["gap_device_long"] == t["gap_jobs"], t
    assert t["gap_device_long"] >= 25 and t["gap_longest"] >= 800, t


def test_default_d_still_takes_the_wide_entry_point(tmp_path):
    """hyper10x300k at the default d = 300 through the shipped binary: its recorded XMFA bytes, and the long form is not used"""
    from parsnp_amd.paths import CORE_BIN
    got, t, _ = widegen.hyper_run(CORE_BIN, "hyper10x300k", tmp_path)
    assert t["gap_device_long"] == 0 and t["gap_jobs_long"] == 0 and t["gap_host"] == 0, t
    assert t["gap_device_narrow"] + t["gap_device_wide"] == t["gap_jobs"] and t["gap_device_wide"] >= 50, t
