"""Gaps of 321 to 1 024 bases between adjacent MUMs -- what a cluster distance d of up to 1 000 leaves -- on the CPU: the host
restatement of the gap aligner (parsnp_amd/csrc/host/gapalign.cpp) against the reference's recorded rows on the long block family
(tests/longgen.py), the whole pipeline at d = 1000 on a set with windows of 330 to 900 bases against the reference binary's
recorded run, and what the long form adds to the C ABI (include/parsnp_mum.h) as far as it needs no device.  The device's side is
tests/test_gpu_long_gaps.py."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import longgen
import widegen
from parsnp_amd.paths import HIP_LIB
from test_gapalign import aligner  # noqa: F401  (fixture: the host restatement)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PM_EINVAL = -2      # include/parsnp_mum.h


def test_host_restatement_on_the_long_family(aligner):  # noqa: F811
    """pins the oracle the GPU test compares against: identical rows on every block of the family, all of which the reference
    aligns itself (a block on which MUSCLE quits comes back as its input, which the check of equal row lengths would catch)"""
    family = longgen.long_blocks()
    wants = longgen.reference_align(family)
    assert len(wants) == len(family) >= 15
    sizes = [len(b) for b in family]
    assert min(sizes) == 2 and max(sizes) == longgen.LONG_SEQS
    assert all(widegen.WIDE_SEQ_LEN < max(len(s) for s in b) <= longgen.LONG_SEQ_LEN and min(len(s) for s in b) >= 1 for b in family)      # every block has a string above 320
    assert [len(s) for s in family[0]] == [321, 321]
    assert any(len(b) > 2 and all(len(s) == longgen.LONG_SEQ_LEN for s in b) for b in family)
    assert any(len(b) == 200 and 850 <= max(len(s) for s in b) <= 950 for b in family)
    assert any("N" in s for b in family for s in b)
    assert all(len(set(b)) <= 50 for b in family)          # the big blocks draw from a few haplotypes
    assert 1700 < max(len(w[0]) for w in wants) <= longgen.LONG_COLS
    for blk, want in zip(family, wants):
        assert len(want) == len(blk) and len({len(r) for r in want}) == 1 and [r.replace("-", "") for r in want] == blk      # the reference aligned it
        assert len(want[0]) <= longgen.LONG_COLS
        assert aligner(blk) == want, (len(blk), blk[0][:40])


def test_long_windows_whole_run_at_d_1000(cpu_checkers, tmp_path):
    """10 genomes of 300 kb with 60 windows of 330 to 900 bases through the CPU build of parsnp_core at d = 1000, 8 threads: the
    reference binary's XMFA bytes and log counters, and the set really has long gaps -- counted by width in the PARSNP_TIMING
    record (on this build every gap is aligned on the host)"""
    got, t = longgen.long_run(cpu_checkers, "long10x300k", tmp_path)
    assert t["gap_jobs_long"] >= 40 and t["gap_longest"] >= 800, t
    assert t["gap_jobs"] >= t["gap_jobs_wide"] >= t["gap_jobs_long"] and t["gap_host"] == t["gap_jobs"], t
    assert t["gap_device_narrow"] == 0 and t["gap_device_wide"] == 0 and t["gap_device_long"] == 0, t


def test_no_long_gap_at_the_default_d(cpu_checkers, tmp_path):
    """the same set at the default d = 300: a window of more than 300 bases ends the cluster, no gap has a string above 320"""
    got, t = longgen.long_run(cpu_checkers, "long10x300k", tmp_path, clusterd=300, reference=None)
    assert t["gap_jobs"] > 0 and t["gap_jobs_long"] == 0 and t["gap_longest"] <= widegen.WIDE_SEQ_LEN, t


def test_new_configs_changed_no_existing_set():
    from parsnp_amd import synth

    def md5(name):
        ref, gs = synth.make(name)
        return hashlib.md5(b"\n".join([ref] + list(gs))).hexdigest()
    from test_tall_gaps import HYPER10_MD5, POP6_MD5
    assert md5("hyper10x300k") == HYPER10_MD5 and md5("pop6x200k") == POP6_MD5
    assert synth.CONFIGS["long10x300k"][1]["n_genomes"] == 10 and synth.CONFIGS["long200x150k"][1]["n_genomes"] == 200
    assert all(synth.CONFIGS[k][1]["windows"]["min_len"] == 330 and synth.CONFIGS[k][1]["windows"]["max_len"] == 900 for k in ("long10x300k", "long200x150k"))


# ---- the C ABI of the long form, as far as it needs no device (the library is cross-compiled by build())

@pytest.fixture(scope="module")
def hip_lib():
    assert os.path.exists(HIP_LIB), "libparsnp_hip.so is not built"
    return C.CDLL(HIP_LIB)


def test_header_declares_and_library_exports_the_long_form():
    hdr = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    assert re.search(r"\bint pm_gap_align_groups_long\(", hdr) and re.search(r"\bint pm_gap_limits_long\(int\* max_seqs, int\* max_seq_len, int\* max_cols\);", hdr)
    assert re.search(r"typedef struct pm_gap_long_stats \{[^}]*jobs_narrow, jobs_wide, jobs_long;[^}]*declined;[^}]*ms_narrow, ms_wide, ms_long;[^}]*\} pm_gap_long_stats;", hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", HIP_LIB], capture_output=True, check=True).stdout.decode()
    for name in ("pm_gap_align_groups_long", "pm_gap_limits_long", "pm_gap_align_groups_wide", "pm_gap_align_groups_tall", "pm_gap_limits", "pm_gap_limits_tall"):
        assert re.search(r" T %s$" % name, syms, re.M), name


def test_limits_need_no_device(hip_lib):
    """pm_gap_limits_long answers (512, 1 024, 2 048); the older limit calls answer what they did"""
    from parsnp_amd.binding import Lib
    assert Lib().gap_limits_long() == (longgen.LONG_SEQS, longgen.LONG_SEQ_LEN, longgen.LONG_COLS) == (512, 1024, 2048)
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    assert hip_lib.pm_gap_limits_long(C.byref(a), None, None) == 0 and a.value == 512      # any pointer may be NULL
    assert hip_lib.pm_gap_limits(C.c_int(0), C.byref(a), C.byref(b), C.byref(c)) == 0 and (a.value, b.value, c.value) == (512, 96, 96)
    assert hip_lib.pm_gap_limits(C.c_int(1), C.byref(a), C.byref(b), C.byref(c)) == 0 and (a.value, b.value, c.value) == (512, 320, 640)
    assert hip_lib.pm_gap_limits_tall(C.byref(a), C.byref(b), C.byref(c)) == 0 and (a.value, b.value, c.value) == (2048, 320, 640)


def test_argument_checks_before_any_device(hip_lib):
    """bad group boundaries are PM_EINVAL, and an empty batch reports every group: both before the call looks for a device"""
    L = hip_lib
    L.pm_gap_align_groups_long.restype = C.c_int
    nseq = np.array([2], np.int32); off = np.array([0, 4, 8], np.int64); chars = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    maxc = np.array([16], np.int32); row_off = np.zeros(1, np.int64); out = np.zeros(33, np.uint8); cols = np.full(1, -7, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    seen = []
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
    cb = CB(lambda ctx, g: seen.append(g))

    def call(n_jobs, group_end):
        ge = np.array(group_end, np.int64)
        return L.pm_gap_align_groups_long(C.c_int(-1), C.c_int64(n_jobs), p(nseq, C.c_int32), p(off, C.c_int64), p(chars, C.c_uint8), p(maxc, C.c_int32),
                                          p(row_off, C.c_int64), p(out, C.c_uint8), C.c_int64(len(out)), p(cols, C.c_int32), C.c_int(len(ge)), p(ge, C.c_int64), cb, None, None)
    assert call(1, [0, 2]) == PM_EINVAL          # the last group does not end at the last job
    assert call(1, [1, 0, 1]) == PM_EINVAL       # a group ends before its predecessor
    assert call(-1, [-1]) == PM_EINVAL
    assert seen == [] and cols[0] == -7
    assert call(0, [0, 0, 0]) == 0 and seen == [0, 1, 2]
