"""GroupedPairEventsWide (parsnp_amd/csrc/engine/store_kernels.h) in the kernel emulation: the small regions the first grouped form
leaves -- more than 32 distinct pieces, more than 8 events of one (piece, strand), more than 1 024 query genomes -- on the designed
batches of tests/groupedwide.py.  Every batch runs with the wide form (group_wide = 1), by default (the wide form is off unless asked for: DESIGN.md 8), with
group_wide = 0 and with group_small = 0, and must give the same
multi-MUMs, every fourth region those of the restatement; the counts of pm_last_timing say which form took the regions.
tests/test_gpu_grouped_wide.py runs the same checks on the device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import groupedwide as G
import oracles
import test_host_logic
import xmfa_util
from conftest import ROOT
from parsnp_amd import driver
from parsnp_amd.binding import Lib, PmError
from parsnp_amd.paths import HIP_LIB

PIECE_CASES = [32, 33, 64, 128, 129]
GENOME_CASES = [(1024, 3), (1025, 4), (2047, 6), (1025, 100), (63, 40), (64, 40), (65, 40)]
DEGENERATE_CASES = ["zero_length", "identical", "all_distinct_128", "no_events"]
WHOLE_RUNS = [(name, wide) for name in ("rearr6x300k", "poprearr10x400k") for wide in ("1", None, "0")]


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


def check_pieces(lib, O, n):
    """exactly n distinct pieces in every region at 200 query genomes: 32 is the first form's, 33 ... 128 the wide form's, 129 nobody's"""
    b = G.piece_batch(100 + n, 200, n)
    assert set(G.distinct_pieces(b)) == {n}
    counts, mums = G.check_batch(lib, O, b)
    print("pieces", n, counts)
    assert mums > 0
    nreg = b.starts.shape[0]
    if n <= 32:
        assert counts["n_grouped_wide"] == 0 and counts["n_grouped"] > 0 and counts["n_handed_back"] == 0, counts
    elif n <= 128:
        assert counts["n_grouped_wide"] > 0 and counts["n_handed_back"] == 0 and counts["n_wide_regions"] == nreg, counts
    else:
        assert counts["n_handed_back"] == nreg and counts["n_grouped_wide"] == 0 and counts["n_grouped"] == 0, counts


def check_events(lib, O):
    """event lists of exactly 9 and exactly 32 (the wide form's) and of 33 (handed back), counted by the restatement"""
    b = G.event_batch(O, 9)
    for r, cs in enumerate(b.info["counts"]):      # the designed counts, once more from the batch's own bytes
        pieces = {b.seqs[g][b.starts[r, g]:b.starts[r, g] + b.lens[r, g]] for g in range(1, len(b.seqs))}
        ref_win = b.seqs[0][b.starts[r, 0]:b.starts[r, 0] + b.lens[r, 0]]
        found = sorted(G.strand_counts(O, ref_win, p, int(b.mins[r])) for p in pieces)
        assert found == sorted(cs) and max(max(c) for c in found) == b.info["wanted"][r], (r, found, cs)
        assert sum(max(c) > 8 for c in found) == 1
    fullest = b.info["wanted"]
    assert 9 in fullest and 32 in fullest and 33 in fullest
    counts, mums = G.check_batch(lib, O, b)
    print("events", counts)
    assert mums > 0
    assert counts["n_handed_back"] == sum(c > 32 for c in fullest) and counts["n_wide_regions"] == sum(8 < c <= 32 for c in fullest), counts
    assert counts["n_grouped_wide"] > 0


def check_genomes(lib, O, nq, n):
    """1 024 query genomes are the first form's; 1 025 and 2 047 the wide form's alone; 63, 64, 65: lanes with none, one or two genomes"""
    b = G.piece_batch(7 * nq + n, nq, n)
    assert set(G.distinct_pieces(b)) == {n}
    counts, mums = G.check_batch(lib, O, b)
    print("genomes", nq, n, counts)
    assert mums > 0 and counts["n_handed_back"] == 0
    if nq > 1024:
        assert counts["n_grouped_wide"] > 0 and counts["n_grouped_wide"] == counts["n_grouped"], counts
    elif n <= 32:
        assert counts["n_grouped_wide"] == 0 and counts["n_grouped"] > 0, counts
    else:
        assert counts["n_grouped_wide"] > 0, counts


def check_degenerate(lib, O, what):
    if what == "zero_length":      # some genomes hold nothing of every third region: the empty piece is one piece more
        b = G.piece_batch(501, 200, 40, zero_len=(3, 17, 64, 200))
        assert set(G.distinct_pieces(b)) == {40, 41}
        counts, mums = G.check_batch(lib, O, b)
        assert counts["n_grouped_wide"] > 0 and counts["n_handed_back"] == 0 and counts["n_wide_regions"] == 16, counts
    elif what == "identical":      # one piece: the first form's
        b = G.piece_batch(502, 50, 1)
        assert set(G.distinct_pieces(b)) == {1}
        counts, mums = G.check_batch(lib, O, b)
        assert mums > 0 and counts["n_grouped_wide"] == 0 and counts["n_grouped"] > 0 and counts["n_handed_back"] == 0, counts
    elif what == "all_distinct_128":      # every genome a piece of its own
        b = G.piece_batch(503, 128, 128)
        assert set(G.distinct_pieces(b)) == {128}
        counts, mums = G.check_batch(lib, O, b)
        assert mums > 0 and counts["n_grouped_wide"] > 0 and counts["n_handed_back"] == 0 and counts["n_wide_regions"] == 16, counts
    else:      # no piece has an event: the regions are taken, their blocks are empty
        b = G.piece_batch(504, 200, 40, minsize=(14, 17), no_events=True)
        counts, mums = G.check_batch(lib, O, b)
        assert mums == 0 and counts["n_wide_regions"] == 16 and counts["n_grouped"] == 0 and counts["n_handed_back"] == 0, counts
    print(what, counts)


def check_sharded(lib, O):
    """two ranks search half of the query genomes each (g_first, g_last: a rank's block holds its own genomes' events, Master.EP
    the pieces its genomes hold) and exchange through host callbacks: the plain session's multi-MUMs on both"""
    from parsnp_amd.binding import Session
    b = G.piece_batch(640, 60, 40)
    with Session(lib, b.seqs) as s:
        s.tune("group_wide", 1)
        plain = s.multi_mum_batch(b.starts, b.lens, b.mins)
        whole = dict(s.last_timing())
    assert sum(len(x[0]) for x in plain) > 0
    ranks = G.sharded_batch(lib, b, 2)
    for got, counts in ranks:
        assert all(G.same(x, y) for x, y in zip(plain, got))
        assert 0 < counts["n_grouped_wide"] < whole["n_grouped_wide"] and counts["n_handed_back"] == 0, (counts, whole)
    assert ranks[0][1]["n_grouped_wide"] + ranks[1][1]["n_grouped_wide"] == whole["n_grouped_wide"]


def check_whole_run(core, name, wide, tmp, threads=4):
    """a rearranged set through parsnp_core with the long-list thresholds lowered: the reference's bytes with the wide form
    (PM_GROUP_WIDE=1), by default and with it switched off"""
    rp, qs, kw = test_host_logic.harsh_inputs(name, str(tmp))
    env = dict(os.environ, PM_DIRTY_MIN="8")
    if wide is not None:
        env["PM_GROUP_WIDE"] = wide
    out = os.path.join(str(tmp), "out")
    rc, _ = driver.run_core(core, rp, qs, out, env=env, threads=threads, **kw)
    assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
    want = test_host_logic.E2E[name]
    assert xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")) == want["xmfa_md5"]
    assert xmfa_util.log_counters(os.path.join(out, "parsnpAligner.log")) == want["log"]


def check_limits(lib):
    assert lib.group_limits(wide=False) == (32, 8, 1024) and lib.group_limits(wide=True) == (128, 32, 2047)
    a = C.c_int()
    assert lib.L.pm_group_limits(C.c_int(1), None, C.byref(a), None) == 0 and a.value == 32      # any pointer may be NULL


@pytest.mark.parametrize("n", PIECE_CASES)
def test_piece_boundaries(libs, n):
    check_pieces(libs[0], libs[1], n)


def test_event_lists(libs):
    check_events(*libs)


@pytest.mark.parametrize("nq,n", GENOME_CASES)
def test_genome_counts(libs, nq, n):
    check_genomes(libs[0], libs[1], nq, n)


@pytest.mark.parametrize("what", DEGENERATE_CASES)
def test_degenerate_regions(libs, what):
    check_degenerate(libs[0], libs[1], what)


def test_sharded_block(libs):
    check_sharded(*libs)


def test_both_wavefront_orders(libs, monkeypatch):
    """the wide launch's wavefronts last to first (PM_EMU_REVERSE_WAVES): they share the block counter and nothing else, so the same
    multi-MUMs and the same counts -- before the kernel meets a device"""
    lib, O = libs
    for b in (G.piece_batch(133, 200, 33), G.piece_batch(228, 200, 128), G.event_batch(O, 9), G.piece_batch(7 * 1025 + 4, 1025, 4)):
        monkeypatch.delenv("PM_EMU_REVERSE_WAVES", raising=False)
        fwd = G.run_three(lib, b)["wide"]
        monkeypatch.setenv("PM_EMU_REVERSE_WAVES", "grouped_pair_events_wide")
        rev = G.run_three(lib, b)["wide"]
        assert all(G.same(x, y) for x, y in zip(fwd[0], rev[0]))
        assert all(fwd[1][k] == rev[1][k] for k in fwd[1] if k.startswith("n_")) and fwd[1]["n_grouped_wide"] > 0


@pytest.mark.parametrize("name,wide", WHOLE_RUNS)
def test_whole_run(emu, tmp_path, name, wide):
    check_whole_run(emu[1], name, wide, tmp_path)


def test_group_limits_and_the_abi(emu, cpu_checkers):
    check_limits(Lib(emu[0]))
    check_limits(Lib(HIP_LIB))      # (cross-compiled by build(); the call needs no device)
    hdr = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    assert re.search(r"\bint pm_group_limits\(int wide, int\* max_pieces, int\* max_events, int\* max_genomes\);", hdr) and '"group_wide"' in hdr
    syms = subprocess.run(["nm", "-D", "--defined-only", HIP_LIB], capture_output=True, check=True).stdout.decode()
    assert re.search(r" T pm_group_limits$", syms, re.M)
    cpu = Lib(os.path.join(ROOT, "oracle", "_ref", "libpm_oracle.so"))      # a provider without the symbol
    with pytest.raises(PmError):
        cpu.group_limits()


def test_unknown_without_the_feature(libs):
    """what the new files rest on: the tune key, and the two counts in pm_last_timing"""
    from parsnp_amd.binding import Session
    b = G.piece_batch(3340, 40, 33)
    with Session(libs[0], b.seqs) as s:
        s.tune("group_wide", 1)
        s.multi_mum_batch(b.starts, b.lens, b.mins)
        counts = dict(s.last_timing())
    assert "n_grouped_wide" in counts and "n_handed_back" in counts and counts["n_grouped_wide"] > 0
    assert len(counts) <= 60      # (Session.last_timing asks for 64 entries)


def test_sanitized_program(tmp_path):
    """tests/emu/grouped_wide_check.cpp: the 33- and 128-piece batches (and a batch of 1 100 genomes) through the wide kernel in the
    emulation, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "grouped_wide_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPM_WAVE_EVENTS=5",
                    os.path.join(ROOT, "tests", "emu", "grouped_wide_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "grouped_wide_check ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
