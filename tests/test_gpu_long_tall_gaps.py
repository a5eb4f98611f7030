"""The long-tall form of the device gap aligner (pm_gap_align_groups_long_tall, include/parsnp_mum.h): gaps of 513 to 2 048 sequences
with a string of 321 to 1 024 bases, up to 2 048 columns, one workgroup of four wavefronts per gap -- what more than 511 query genomes
run with a cluster distance d of up to 1 000 produce.  The bar is the reference's rows (libMUSCLE through oracle/_ref/muscle_ref,
recorded in tests/golden/muscle_long_tall_runs.json.xz and gapalign.json) and the reference binary's whole run at d = 1000
(tests/golden/long_tall_gap_runs.json.xz); a job is declined (cols = -1) exactly when it lies outside pm_gap_limits_long_tall, and no
job of the long-tall family is."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gapgen
import longgen
import longtallgen
import tallgen
import widegen
from parsnp_amd.paths import HIP_LIB
from test_gpu_long_gaps import LongStats
from test_gpu_long_gaps import align as align_long
from test_gpu_tall_gaps import TallStats
from test_gpu_tall_gaps import align as align_tall
from test_gpu_wide_gaps import capacity, inside

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(HIP_LIB)
    L.pm_gap_align_batch.restype = C.c_int
    L.pm_gap_align_groups_wide.restype = C.c_int
    L.pm_gap_align_groups_tall.restype = C.c_int
    L.pm_gap_align_groups_long.restype = C.c_int
    L.pm_gap_last_error.restype = C.c_char_p
    assert hasattr(L, "pm_gap_align_groups_long_tall") and hasattr(L, "pm_gap_limits_long_tall"), "this library has no long-tall form of the gap aligner"
    L.pm_gap_align_groups_long_tall.restype = C.c_int
    return L


def limits_long_tall(L):
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    assert L.pm_gap_limits_long_tall(C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


def align(L, blocks, maxc, group_end=None, on_group=None):
    """pm_gap_align_groups_long_tall -> (per block: list of rows, or None where the device declined; the call's statistics)"""
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
    st = longtallgen.LongTallStats()

    def rows_of(j):
        if cols[j] < 0:
            return None
        base, w = int(row_off[j]), int(maxc[j])
        return [out[base + i * w: base + i * w + int(cols[j])].tobytes().decode() for i in range(len(blocks[j]))]

    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
    cb = CB(lambda ctx, g: on_group(g, [rows_of(j) for j in range(0 if g == 0 else int(group_end[g - 1]), int(group_end[g]))]) if on_group else None)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    rc = L.pm_gap_align_groups_long_tall(C.c_int(-1), C.c_int64(len(blocks)), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32),
                                         p(row_off, C.c_int64), p(out, C.c_uint8), C.c_int64(len(out)), p(cols, C.c_int32), C.c_int(len(group_end)),
                                         p(group_end, C.c_int64), cb, None, C.byref(st))
    assert rc == 0, L.pm_gap_last_error()
    assert all(c == -1 or c >= 1 for c in cols)
    return [rows_of(j) for j in range(len(blocks))], st


def test_limits_are_the_documented_ones(lib):
    assert limits_long_tall(lib) == (longtallgen.LT_SEQS, longtallgen.LT_SEQ_LEN, longtallgen.LT_COLS) == (2048, 1024, 2048)


def test_long_tall_blocks_and_committed_vectors_against_the_reference(lib):
    """the long-tall family and every committed vector of the narrow tests in ONE call: the reference's rows for every block inside
    the limits, cols = -1 exactly for those outside; none of the family is declined, and all of it runs in the long-tall form"""
    lim = limits_long_tall(lib)
    cs, family_rows = longtallgen.family()
    family = [c.block for c in cs]
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "gapalign.json")))
    blocks = family + [b["in"] for b in data]
    wants = family_rows + [b["out"] for b in data]
    maxc = [longtallgen.capacity(b) for b in family] + [capacity(b["in"], lim[2]) for b in data]
    got, st = align(lib, blocks, maxc)
    declined = 0
    for k, (blk, want, rows, cap) in enumerate(zip(blocks, wants, got, maxc)):
        if inside(blk, want, lim) and len(want[0]) <= cap:
            assert rows == want, (k, len(blk), blk[0][:40])
        else:
            assert rows is None, (k, len(blk), blk[0][:40])
            declined += 1
            assert k >= len(family), "a block of the long-tall family was declined"
    assert all(r is not None for r in got[:len(family)])
    assert st.jobs_long_tall == len(family) and st.declined == declined
    assert st.jobs_narrow + st.jobs_wide + st.jobs_tall + st.jobs_long + st.jobs_long_tall + st.declined == len(blocks)
    assert st.jobs_narrow > 200 and st.jobs_tall == 0 and st.ms_long_tall > 0


def test_declines_and_the_sentinel(lib):
    """the exact decline predicate on the device, with out_bytes exact and one byte short: only the aligned jobs' areas are written"""
    jobs = longtallgen.decline_jobs()
    st, expect = longtallgen.run_call(lib, jobs)
    assert expect == dict(narrow=0, wide=0, tall=0, long=0, long_tall=2, declined=4)
    st, expect = longtallgen.run_call(lib, jobs, short_by=1)
    assert expect == dict(narrow=0, wide=0, tall=0, long=0, long_tall=1, declined=5)


def test_five_forms_in_five_groups_match_single_jobs(lib):
    """narrow, wide, tall, long and long-tall jobs interleaved in one call, in five groups with a `done` callback -- one group of
    long-tall jobs only, one holding only a 2 049-sequence job and a job with a 1 025-base string among 600 (both declined): the rows
    of one job per call, every group reported in order with its rows in place"""
    lim = limits_long_tall(lib)
    lt = [c.block for c in longtallgen.long_tall_blocks()[:4]]
    long_ = [b for b in longgen.long_blocks() if len(b) <= 50][:4]
    tall = [b for b in tallgen.tall_blocks() if max(len(s) for s in b) <= 100 and len(b) <= 601][:3]
    wide = [b for b in widegen.wide_blocks() if len(b) <= 50][:6]
    narrow = gapgen.blocks(80, 30, lengths=(2, 5, 13, 30, 60, 90))
    too_many = [lt[0][1]] * (lim[0] + 1)
    too_long = [lt[1][i % len(lt[1])] for i in range(599)] + ["A" * (lim[1] + 1)]
    assert len(long_) == 4 and len(tall) == 3 and len(wide) == 6
    blocks = narrow[:10] + [lt[0]] + wide[:3] + [long_[0], tall[0]] + narrow[10:20] + [long_[1]] + lt[1:3] + [too_many, too_long] + wide[3:6] + [tall[1], long_[2], lt[3]] + narrow[20:] + [tall[2], long_[3]]
    group_end = [16, 27, 29, 31, len(blocks)]
    assert blocks[27:29] == lt[1:3] and blocks[29:31] == [too_many, too_long]
    maxc = [longtallgen.capacity(b) if max(len(s) for s in b) > widegen.WIDE_SEQ_LEN else capacity(b, 640) for b in blocks]
    single = [align(lib, [b], [c])[0][0] for b, c in zip(blocks, maxc)]
    assert all(s is None for s in single[29:31]) and sum(s is None for s in single) == 2
    seen = []
    got, st = align(lib, blocks, maxc, group_end=group_end,
                    on_group=lambda g, rows: seen.append((g, rows == single[(0 if g == 0 else group_end[g - 1]):group_end[g]])))
    assert seen == [(g, True) for g in range(5)]
    assert got == single
    assert st.declined == 2 and st.jobs_long_tall == 4 and st.jobs_long == 4 and st.jobs_tall == 3 and st.jobs_wide >= 6 and st.jobs_narrow + st.jobs_wide == 36
    assert st.ms_long_tall > 0 and st.ms_long > 0 and st.ms_tall > 0 and st.ms_wide > 0 and st.ms_narrow > 0


def test_older_entry_points_keep_their_limits(lib):
    """the 513 x 321 block comes back -1 from pm_gap_align_groups_tall and pm_gap_align_groups_long, beside a job they take"""
    blk = longtallgen.long_tall_blocks()[0].block
    assert len(blk) == widegen.WIDE_SEQS + 1 and max(len(s) for s in blk) == widegen.WIDE_SEQ_LEN + 1
    small = [blk[0][:300], blk[0][10:290]]
    got, st = align_tall(lib, [blk, small], [400, 640])
    assert got[0] is None and got[1] is not None
    assert isinstance(st, TallStats) and st.declined == 1 and st.jobs_wide == 1 and st.jobs_tall == 0
    got, st = align_long(lib, [blk, small], [400, 640])
    assert got[0] is None and got[1] is not None
    assert isinstance(st, LongStats) and st.declined == 1 and st.jobs_wide == 1 and st.jobs_long == 0


def test_six_hundred_genomes_with_long_windows_on_device(tmp_path):
    """parsnp_core as shipped at d = 1000, 16 threads, on the set of tests/test_long_tall_gaps.py: the reference binary's XMFA bytes and
    log counters, and no gap is aligned on the host -- the windows' gaps of 601 sequences go to the long-tall form"""
    from parsnp_amd.paths import CORE_BIN
    got, t = longtallgen.long_tall_run(CORE_BIN, "longtall600x60k", tmp_path)
    assert t["gap_host"] == 0 and t["gap_device_long_tall"] >= 5 and t["gap_longest"] >= 800, t
    assert t["gap_device_narrow"] + t["gap_device_wide"] + t["gap_device_tall"] + t["gap_device_long"] + t["gap_device_long_tall"] == t["gap_jobs"], t
    assert t["gap_device_long"] == 0 and t["gap_jobs_long"] >= t["gap_device_long_tall"], t


def test_default_d_still_takes_the_tall_entry_point(tmp_path):
    """tall640x100k at the default d = 300 through the shipped binary: its recorded XMFA bytes, all gaps in the forms of
    pm_gap_align_groups_tall, and the long-tall form is not used"""
    from parsnp_amd.paths import CORE_BIN
    got, t = tallgen.tall_run(CORE_BIN, "tall640x100k", tmp_path)
    assert t["gap_device_long_tall"] == 0 and t["gap_device_long"] == 0 and t["gap_jobs_long"] == 0 and t["gap_host"] == 0, t
    assert t["gap_device_narrow"] + t["gap_device_wide"] + t["gap_device_tall"] == t["gap_jobs"] and t["gap_device_tall"] >= 300, t
