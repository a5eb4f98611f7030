"""The index build by buckets in LDS (parsnp_amd/csrc/engine/index_kernels.h) in the kernel emulation: the cases of tests/indexgen.py
with `index_build` = 1 against `index_build` = 0 (IndexInsert for every region) and against the restatement, the counts of
pm_last_timing, IndexVerify's verdict on both tables.  The emulation runs a bucket's records one after another; what only a
wavefront does -- the runs over neighbouring lanes, the compare-and-swap in LDS -- runs in tests/test_gpu_index_buckets.py."""
import os
import subprocess

import pytest

import indexgen as G
import oracles
import test_emu_engine as T
from conftest import ROOT
from parsnp_amd.binding import Lib, PmError, Session


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


def test_probe_seeds():
    """what the two probe cases were chosen for, by the restatement of the fill's probe runs: records reach their bucket's end in
    both, and in the first one of the last bucket does -- IndexOverflow's loop takes it round the region's end"""
    c = G.probe_small()
    total, last = G.overflow_model(c.ref, 16, slot_factor=1)
    assert total > 0 and last > 0, (total, last)
    assert G.table_shape(1000, slot_factor=1)[:3] == (1024, 8192, 9)
    total, _ = G.overflow_model(G.probe_default().ref, 16)
    assert total > 0


@pytest.mark.parametrize("name", [n for n in G.CASES if n not in G.DEGENERATE and not n.endswith("_short")])
def test_case(libs, name):
    G.check(libs[0], libs[1], G.CASES[name]())


@pytest.mark.parametrize("name", G.DEGENERATE)
def test_one_kmer_for_nearly_everything(libs, emu, name):
    """20 000 N, a 20 000-base homopolymer, 2 000 copies of a period-7 unit in 40 kb: one K-mer (or seven) for nearly every record.
    Under G.watchdog: today's build first, in a process of its own, then the bucket build within that time + G.WATCHDOG_MARGIN_S.
    The emulation runs these lengths with a work budget of 2^14 for both builds: at the default budget (2^22) it spends its time in
    RepeatLength's quadratic chain walks, one thread after another -- measured for this test as first written, both builds and the
    restatement: 23 s (all_n), 23 s (homopolymer), 142 s (tandem); the device test runs them at the default budget in under a second
    each.  With 2^14 RepeatLength gives the walks up at once and the region takes the suffix-array path; the index is still built,
    verified (IndexVerify walks every chain) and walked by the search.  The default budget with RepeatLength's walks over the
    bucket-built chains runs in the emulation at a fifth of the length: test_one_kmer_default_budget."""
    G.watchdog(emu[0], name, {"work_budget": 1 << 14})
    G.check(libs[0], libs[1], G.CASES[name](), more_tunes={"work_budget": 1 << 14})


@pytest.mark.parametrize("name", [n + "_short" for n in G.DEGENERATE])
def test_one_kmer_default_budget(libs, emu, name):
    """4 000 N, a 4 000-base homopolymer, 400 copies of the period-7 unit in 8 kb at the default work budget, under the same watchdog"""
    G.watchdog(emu[0], name)
    t, _, _ = G.check(libs[0], libs[1], G.CASES[name]())
    assert "dense_regions" not in t or name == "tandem_short", t      # (RepeatLength walked the chains; the tandem array may still exceed the budget)


def test_mixed_batch(libs):
    G.check_mixed(libs[0], libs[1], T)


def test_overflow_counts_match_the_model(libs):
    """random 16-mers are distinct, so the records that reach their bucket's end are the same in any order: the model's count"""
    for c, sf in ((G.probe_small(), 1), (G.probe_default(), 2)):
        t = G.run_whole(libs[0], c, 1)[1]
        assert t["index_overflow"] == G.overflow_model(c.ref, 16, slot_factor=sf)[0]


def test_environment_tune(libs):
    """PARSNP_TUNE reaches the sessions that entry points open for themselves: index_build = 0 there means no position by buckets; a
    key the engine does not know fails the session's creation"""
    c = G.region_end()
    os.environ["PARSNP_TUNE"] = "index_build=0,index_bucket_min=1"
    try:
        with Session(libs[0], [c.ref] + c.qs) as s:
            s.whole(16)
            assert dict(s.last_timing())["index_bucketed"] == 0
        os.environ["PARSNP_TUNE"] = "index_build=1,index_bucket_min=1"
        with Session(libs[0], [c.ref] + c.qs) as s:
            s.whole(16)
            assert dict(s.last_timing())["index_bucketed"] == len(c.ref)
        os.environ["PARSNP_TUNE"] = "index_build=1,no_such_key=1"
        with pytest.raises(PmError):
            Session(libs[0], [c.ref] + c.qs)
    finally:
        del os.environ["PARSNP_TUNE"]


def test_documented():
    hdr = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    for word in ('"index_build"', '"index_bucket_min"', '"index_verify"', '"index_overflow_cap"', "index_bucketed", "index_overflow", "index_lost", "PARSNP_TUNE"):
        assert word in hdr, word


def test_sanitized_program(libs, tmp_path):
    """tests/emu/index_buckets_check.cpp: every case of indexgen.CASES at its full length and the mixed batch (G.write_cases: inputs,
    the restatement's multi-MUMs, the emulation's counts) through the emulation as a program of its own under AddressSanitizer and
    UndefinedBehaviorSanitizer, by both builds: the restatement's multi-MUMs, index_lost = 0, the same counts"""
    cases = str(tmp_path / "cases.txt")
    G.write_cases(cases, libs[0], libs[1], T)
    exe = str(tmp_path / "index_buckets_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPM_WAVE_EVENTS=5",
                    os.path.join(ROOT, "tests", "emu", "index_buckets_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, cases], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "index_buckets_check ok: %d cases" % (len(G.CASES) + 1) in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
