"""Gaps of more than 512 sequences WITH a string of more than 320 bases -- more than 511 query genomes run at a raised cluster
distance d -- on the CPU: the host restatement of the gap aligner (parsnp_amd/csrc/host/gapalign.cpp) against the reference's
recorded rows on the long-tall block family (tests/longtallgen.py); the long-tall form of the device kernel itself, executed on the
host by tests/emu/gap_emu.cpp (gapalign_hip.hip compiled unchanged, a fiber per lane) under an ascending and a descending schedule,
on the cheap blocks and the declines; what the form adds to the C ABI (include/parsnp_mum.h) as far as it needs no device; and the
whole pipeline at d = 1000 on a set of 600 genomes against the reference binary's recorded run.  The device's side is
tests/test_gpu_long_tall_gaps.py."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import pytest

import longtallgen
from parsnp_amd.paths import HIP_LIB
from test_gap_edges import SCHEDULES, emu_long  # noqa: F401  (fixture: the kernel's source compiled for the host)
from test_gapalign import aligner  # noqa: F401  (fixture: the host restatement)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_restatement_on_the_long_tall_family(aligner):  # noqa: F811
    """pins the oracle the GPU test compares against: identical rows on every block of the family, all of which the reference
    aligns itself, inside 2 048 columns and inside the writer's row capacity -- "no block of the family is declined" is then a
    statement about the kernel, not about the inputs"""
    cs, wants = longtallgen.family()
    assert [c.name for c in cs] == ["first", "rounds 576", "rounds 577", "rounds 640", "distinct 700", "far corner", "whole run"]
    assert [len(c.block) for c in cs] == [513, 576, 577, 640, 700, 2048, 2001]
    assert all(longtallgen.OLD_SEQS < len(c.block) <= longtallgen.LT_SEQS and longtallgen.OLD_SEQ_LEN < max(len(s) for s in c.block) <= longtallgen.LT_SEQ_LEN
               and min(len(s) for s in c.block) >= 1 for c in cs)
    first = cs[0].block
    assert sorted(len(s) for s in first)[-2:] == [40, 321] and len(set(first)) == 513 and min(len(s) for s in first) == 1
    assert all(max(len(s) for s in c.block) == 400 and sum(len(s) > 40 for s in c.block) == 1 and len(set(c.block)) <= longtallgen.HAPLOTYPES + 1 for c in cs[1:4])
    assert len(set(cs[4].block)) == 700 and all(330 <= len(s) <= 360 for s in cs[4].block)
    assert max(len(s) for s in cs[5].block) == longtallgen.LT_SEQ_LEN and len(set(cs[5].block)) == longtallgen.HAPLOTYPES + 1
    assert all(850 <= len(s) <= 950 for s in cs[6].block) and len(set(cs[6].block)) == longtallgen.HAPLOTYPES
    assert len(wants[5][0]) > 1024      # the far corner: columns beyond the longest string
    for c, want in zip(cs, wants):
        blk = c.block
        assert len(want) == len(blk) and len({len(r) for r in want}) == 1 and [r.replace("-", "") for r in want] == blk, c.name      # the reference aligned it
        assert len(want[0]) <= min(longtallgen.LT_COLS, longtallgen.capacity(blk)), c.name
        assert aligner(blk) == want, c.name


# ---- the long-tall form, executed on the host

def _emu(emu, descending):
    assert hasattr(emu, "pm_gap_align_groups_long_tall"), "the kernel's source has no long-tall entry point"
    emu.gap_emu_set_schedule(descending)
    return emu


def _job(k):
    cs, rows = longtallgen.family()
    return longtallgen.Job(cs[k].block, len(rows[k][0]) + k % 3, rows[k], cs[k].name)


@SCHEDULES
def test_emulated_first_block(emu_long, descending):  # noqa: F811
    """513 sequences, one of 321 bases: the first job beyond both older limits, alone in its call"""
    st, expect = longtallgen.run_call(_emu(emu_long, descending), [_job(0)])
    assert expect["long_tall"] == 1 and expect["declined"] == 0


@SCHEDULES
def test_emulated_round_boundaries(emu_long, descending):  # noqa: F811
    """576, 577 and 640 sequences in one call: the merge's rounds of 64 and the 256-thread loops at their boundaries"""
    st, expect = longtallgen.run_call(_emu(emu_long, descending), [_job(1), _job(2), _job(3)])
    assert expect["long_tall"] == 3 and expect["declined"] == 0


@SCHEDULES
def test_emulated_declines(emu_long, descending):  # noqa: F811
    """the exact decline predicate, with out_bytes exact and one byte short; the sentinel stays in every declined job's rows"""
    emu = _emu(emu_long, descending)
    jobs = longtallgen.decline_jobs()
    st, expect = longtallgen.run_call(emu, jobs)
    assert expect == dict(narrow=0, wide=0, tall=0, long=0, long_tall=2, declined=4)
    st, expect = longtallgen.run_call(emu, jobs, short_by=1)
    assert expect == dict(narrow=0, wide=0, tall=0, long=0, long_tall=1, declined=5)


def test_emulated_older_entry_points_decline_the_first_block(emu_long):  # noqa: F811
    """pm_gap_align_groups_long and _tall answer -1 for 513 x 321, as they always have, before any launch"""
    import numpy as np
    blk = longtallgen.family()[0][0].block
    nseq = np.array([len(blk)], np.int32)
    off = np.zeros(len(blk) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in blk])
    chars = np.frombuffer("".join(blk).encode(), np.uint8).copy()
    maxc = np.array([400], np.int32); ro = np.zeros(1, np.int64); ge = np.array([1], np.int64)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    for entry in ("long", "tall"):
        out = np.full(len(blk) * 400, longtallgen.SENTINEL, np.uint8)
        cols = np.full(1, -7, np.int32)
        fn = getattr(emu_long, "pm_gap_align_groups_" + entry)
        fn.restype = C.c_int
        assert fn(C.c_int(-1), C.c_int64(1), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32), p(ro, C.c_int64), p(out, C.c_uint8),
                  C.c_int64(len(out)), p(cols, C.c_int32), C.c_int(1), p(ge, C.c_int64), None, None, None) == 0
        assert cols[0] == -1 and (out == longtallgen.SENTINEL).all(), entry


# ---- the C ABI of the long-tall form, as far as it needs no device (the library is cross-compiled by build())

def test_header_declares_and_library_exports_the_long_tall_form():
    hdr = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    assert re.search(r"\bint pm_gap_align_groups_long_tall\(", hdr) and re.search(r"\bint pm_gap_limits_long_tall\(int\* max_seqs, int\* max_seq_len, int\* max_cols\);", hdr)
    assert re.search(r"typedef struct pm_gap_long_tall_stats \{[^}]*jobs_narrow, jobs_wide, jobs_tall, jobs_long, jobs_long_tall;[^}]*declined;"
                     r"[^}]*ms_narrow, ms_wide, ms_tall, ms_long, ms_long_tall;[^}]*\} pm_gap_long_tall_stats;", hdr)
    assert "outside every form" not in hdr      # no corner of 2 048 x 1 024 stays on the host
    syms = subprocess.run(["nm", "-D", "--defined-only", HIP_LIB], capture_output=True, check=True).stdout.decode()
    for name in ("pm_gap_align_groups_long_tall", "pm_gap_limits_long_tall", "pm_gap_align_groups_long", "pm_gap_limits_long", "pm_gap_align_groups_tall", "pm_gap_limits_tall"):
        assert re.search(r" T %s$" % name, syms, re.M), name


def test_limits_need_no_device():
    """pm_gap_limits_long_tall answers (2 048, 1 024, 2 048); the older limit calls answer what they did"""
    from parsnp_amd.binding import Lib
    lib = Lib()
    assert lib.gap_limits_long_tall() == (longtallgen.LT_SEQS, longtallgen.LT_SEQ_LEN, longtallgen.LT_COLS) == (2048, 1024, 2048)
    assert lib.gap_limits_tall() == (2048, 320, 640) and lib.gap_limits_long() == (512, 1024, 2048)
    assert lib.gap_limits(wide=True) == (512, 320, 640) and lib.gap_limits(wide=False) == (512, 96, 96)
    L = C.CDLL(HIP_LIB)
    a = C.c_int()
    assert L.pm_gap_limits_long_tall(None, C.byref(a), None) == 0 and a.value == 1024      # any pointer may be NULL


def test_statistics_records_keep_their_sizes():
    assert C.sizeof(longtallgen.LongTallStats) == 11 * 8
    from test_gap_edges import LongStats, Stats, TallStats
    assert (C.sizeof(Stats), C.sizeof(TallStats), C.sizeof(LongStats)) == (40, 56, 56)


# ---- the whole run

def test_new_config_changed_no_existing_set():
    from parsnp_amd import synth

    def md5(name):
        ref, gs = synth.make(name)
        return hashlib.md5(b"\n".join([ref] + list(gs))).hexdigest()
    from test_tall_gaps import HYPER10_MD5, POP6_MD5
    assert md5("hyper10x300k") == HYPER10_MD5 and md5("pop6x200k") == POP6_MD5
    cfg = synth.CONFIGS["longtall600x60k"][1]
    assert cfg["n_genomes"] == 600 and cfg["n"] == 60_000 and cfg["windows"] == dict(count=6, haplotypes=24, min_len=330, max_len=900)


def test_six_hundred_genomes_with_long_windows_whole_run(cpu_checkers, tmp_path):
    """600 genomes of 60 kb with 6 windows of 330 to 900 bases (24 haplotypes) through the CPU build of parsnp_core at d = 1000, 16
    threads: the reference binary's XMFA bytes and log counters; every gap has 601 sequences and (on this build) is aligned on the host"""
    got, t = longtallgen.long_tall_run(cpu_checkers, "longtall600x60k", tmp_path)
    assert t["gap_jobs_long"] >= 5 and t["gap_longest"] >= 800, t
    assert t["gap_host"] == t["gap_jobs"] and t["gap_device_long"] == 0 and t.get("gap_device_long_tall", 0) == 0, t
