"""The wide form of the device gap aligner (pm_gap_align_groups_wide, include/parsnp_mum.h): gaps of up to 320 bases and 640
columns, what the reference's default cluster distance d = 300 produces.  The bar is the reference's rows (libMUSCLE through
oracle/_ref/muscle_ref, recorded in tests/golden/muscle_wide_runs.json.xz and tests/golden/gapalign.json) and the reference
binary's whole runs (tests/golden/wide_gap_runs.json.xz); a job is declined (cols = -1) exactly when it lies outside
pm_gap_limits(1, ...)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gapgen
import widegen
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stats(C.Structure):
    _fields_ = [("jobs_narrow", C.c_int64), ("jobs_wide", C.c_int64), ("declined", C.c_int64), ("ms_narrow", C.c_double), ("ms_wide", C.c_double)]


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(HIP_LIB)
    L.pm_gap_align_batch.restype = C.c_int
    L.pm_gap_last_error.restype = C.c_char_p
    return L


def limits(L, wide):
    assert hasattr(L, "pm_gap_align_groups_wide") and hasattr(L, "pm_gap_limits"), "this library has no wide form of the gap aligner"
    L.pm_gap_align_groups_wide.restype = C.c_int
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    assert L.pm_gap_limits(C.c_int(wide), C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


def capacity(block, most):
    return min(most, 2 * max(len(s) for s in block) + 16)


def align(L, blocks, maxc, group_end=None, on_group=None, entry="wide"):
    """-> (per block: list of rows, or None where the device declined; the call's statistics)"""
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
    st = Stats()

    def rows_of(j):
        if cols[j] < 0:
            return None
        base = int(row_off[j])
        return [out[base + i * int(maxc[j]): base + i * int(maxc[j]) + int(cols[j])].tobytes().decode() for i in range(len(blocks[j]))]

    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
    cb = CB(lambda ctx, g: on_group(g, [rows_of(j) for j in range(0 if g == 0 else int(group_end[g - 1]), int(group_end[g]))]) if on_group else None)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    if entry == "batch":
        rc = L.pm_gap_align_batch(C.c_int(-1), C.c_int64(len(blocks)), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32),
                                  p(row_off, C.c_int64), p(out, C.c_uint8), C.c_int64(len(out)), p(cols, C.c_int32))
    else:
        rc = L.pm_gap_align_groups_wide(C.c_int(-1), C.c_int64(len(blocks)), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32),
                                        p(row_off, C.c_int64), p(out, C.c_uint8), C.c_int64(len(out)), p(cols, C.c_int32), C.c_int(len(group_end)),
                                        p(group_end, C.c_int64), cb, None, C.byref(st))
    assert rc == 0, L.pm_gap_last_error()
    return [rows_of(j) for j in range(len(blocks))], st


def inside(block, want, lim):
    """the block lies inside the limits `lim` = (sequences, bases, columns), with an alphabet the device's row coding round-trips
    (upper case without 'U': include/parsnp_mum.h); want: the reference's rows"""
    seqs, bases, columns = lim
    return (2 <= len(block) <= seqs and all(0 < len(s) <= bases for s in block) and len(want[0]) <= columns
            and not any(ch.islower() or ch == "U" for s in block for ch in s))


def test_limits_are_the_documented_ones(lib):
    assert limits(lib, 0) == (512, widegen.NARROW_COLS, widegen.NARROW_COLS)
    assert limits(lib, 1) == (widegen.WIDE_SEQS, widegen.WIDE_SEQ_LEN, widegen.WIDE_COLS)


def test_wide_blocks_and_committed_vectors_against_the_reference(lib):
    """every block of the wide family and every committed vector of the narrow tests: the reference's rows for the blocks inside the
    wide limits, cols = -1 exactly for those outside; none of the wide family is declined"""
    lim = limits(lib, 1)
    family = widegen.wide_blocks()
    wants = widegen.reference_align(family)
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "gapalign.json")))
    blocks = family + [b["in"] for b in data]
    wants = wants + [b["out"] for b in data]
    got, st = align(lib, blocks, [capacity(b, lim[2]) for b in blocks])
    declined = 0
    for k, (blk, want, rows) in enumerate(zip(blocks, wants, got)):
        if inside(blk, want, lim) and len(want[0]) <= capacity(blk, lim[2]):
            assert rows == want, (k, len(blk), blk[0][:40])
        else:
            assert rows is None, (k, len(blk), blk[0][:40])
            declined += 1
            assert k >= len(family), "a block of the wide family was declined"
    assert all(r is not None for r in got[:len(family)])
    assert st.declined == declined and st.jobs_narrow + st.jobs_wide == len(blocks) - declined
    assert st.jobs_wide >= len(family) and st.jobs_narrow > 200


def test_mixed_groups_match_single_jobs(lib):
    """narrow and wide jobs mixed in one call, in five groups with a `done` callback -- one group of wide jobs only, one of a
    512-sequence wide job whose rows do not fit the LDS, one of declined jobs only: the rows of one job per call, every group
    reported in order with its rows in place"""
    lim = limits(lib, 1)
    family = widegen.wide_blocks()
    narrow = gapgen.blocks(77, 60, lengths=(2, 5, 13, 30, 60, 90))
    big = next(b for b in family if len(b) == lim[0])
    wide_only = [b for b in family if len(b) <= 50][:8]
    blocks = narrow[:30] + family[:6] + wide_only + [big] + [["A" * (lim[1] + 1), "ACGT"]] * 2 + narrow[30:] + family[6:12]
    group_end = [36, 44, 45, 47, len(blocks)]
    maxc = [capacity(b, lim[2]) for b in blocks]
    assert len(big) * maxc[44] + 60 * 1024 > 160 * 1024      # its rows alone are more than the LDS left beside the fixed block
    single = [align(lib, [b], [c])[0][0] for b, c in zip(blocks, maxc)]
    assert all(s is None for s in single[45:47]) and sum(s is None for s in single) == 2
    seen = []
    got, st = align(lib, blocks, maxc, group_end=group_end,
                    on_group=lambda g, rows: seen.append((g, rows == single[(0 if g == 0 else group_end[g - 1]):group_end[g]])))
    assert seen == [(g, True) for g in range(5)]
    assert got == single
    assert st.declined == 2 and st.jobs_wide >= 6 + 8 + 1 + 6 and st.jobs_narrow >= 50
    assert st.ms_wide > 0 and st.ms_narrow > 0


def test_narrow_entry_points_keep_their_limits(lib):
    """pm_gap_align_batch still answers -1 for a 97-base sequence: the two narrow entry points keep the limits they had"""
    rng_block = [["A" * 97, "A" * 60], ["ACGT" * 24 + "A", "ACGT" * 24], ["ACGT" * 24, "ACGT" * 23]]
    got, _ = align(lib, rng_block, [200, 200, 96], entry="batch")
    assert got[0] is None and got[1] is None and got[2] is not None


def test_hypervariable_windows_whole_run_on_device(tmp_path):
    """parsnp_core as shipped, default settings, on the set of tests/test_wide_gaps.py: the reference binary's XMFA bytes and log
    counters, and no gap is aligned on the host -- the 160 windows go to the wide form"""
    from parsnp_amd.paths import CORE_BIN
    got, t, _ = widegen.hyper_run(CORE_BIN, "hyper10x300k", tmp_path)
    assert t["gap_host"] == 0 and t["gap_device_wide"] >= 50, t
    assert t["gap_jobs_wide"] >= 50 and t["gap_longest"] >= 250 and t["gap_device_narrow"] + t["gap_device_wide"] == t["gap_jobs"], t


def test_two_hundred_genomes_with_windows(tmp_path):
    """200 genomes of 200 kb with 100 windows of 24 haplotypes each, 16 threads: the reference binary's recorded XMFA bytes and log
    counters, every gap on the device"""
    from parsnp_amd.paths import CORE_BIN
    got, t, _ = widegen.hyper_run(CORE_BIN, "hyper200x200k", tmp_path, threads=16)
    assert t["gap_host"] == 0 and t["gap_device_wide"] >= 50 and t["gap_longest"] >= 250, t
