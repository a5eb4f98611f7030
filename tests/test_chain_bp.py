"""Phases C-D on the device for a diagonal difference given in bases (`--max-diagonal-difference 100bp`: diagdiff > 1 in the ini),
in the kernel emulation; tests/test_gpu_chain_bp.py runs the same checks on the device.

Call level: the designed lists of tests/chainbp.py through pm_store_chain_begin / _end -- the row list, the byte per MUM (0 member,
1 head, 2 in no LCB), pm_chain_info, pm_store_chain_passed and the layout afterwards against the sequential restatement of the
recurrence.  End to end: small sets with indels of several bases through parsnp_core, three steps in one process, against the
bytes and log counters the REFERENCE binary left in tests/golden/e2e_chain_bp.json (tests/golden/make_chain_bp_golden.py), with
the chain on the device (`chain=1` in the route log) and with the host's list logic (PARSNP_NO_DEVICE_CHAIN).

Without the feature the route assertion (test_end_to_end: `chain=1` with diagdiff in bases), the lists of test_designed_list whose
MUMs are passed (the ratio test was applied to diag_diff > 1) and test_the_abi (pm_store_chain_passed) fail."""
import json
import os
import re
import subprocess
import sys

import pytest

import chainbp as cb
import storecalls as sc
import xmfa_util
from conftest import ROOT
from parsnp_amd import driver, synth
from parsnp_amd.binding import Lib, PmError, Session
from parsnp_amd.paths import HIP_LIB

GOLDEN = os.path.join(ROOT, "tests", "golden", "e2e_chain_bp.json")


@pytest.fixture(scope="module")
def lib(emu):
    return Lib(emu[0])


# ------------------------------------------------------------------------------------------------------------------ call level
def check_floors(name, w):
    """the paths a list was designed for, where the runs of passed MUMs (asserted by chainbp.check_case) do not say it all"""
    P, J, C_ = cb.PASS, cb.JOIN, cb.CLOSE
    if name in ("bar2", "bar25"):
        D = cb.CASES[name][3]
        m = w.model
        seen = {}
        for x in range(1, len(w.rows1)):
            g = m.gaps(w.rows1[x], w.rows1[w.b1[x]])
            if w.b1[x] == x - 1:
                seen[(min(g), max(g))] = w.v1[x]
        for gaps, v in {(3, D + 2): J, (3, D + 3): P, (3, D + 4): P, (0, D): J, (0, D + 1): P}.items():
            assert seen.get(gaps) == v, "%s: gaps %s -> %s" % (name, gaps, seen.get(gaps))
    if name == "no_pass":
        assert w.passed == (0, 0) and w.info["n_lcbs"] == 2
    if name == "pass_at_1":
        assert w.v1[1] == P
    if name == "pass_last":
        assert w.v1[-1] == P and w.heads[-1] == 2
    if name == "pass_after_head":
        x = w.v1.index(P)
        assert w.v1[x - 1] == C_ and x - 1 > 0
    if name.startswith("meet_after"):
        (x1, p1, _), (x2, _, _) = w.win1
        assert x2 == x1 + p1 + 1, "the second run does not begin right behind the MUM that ends the first"
    if name == "start_inside":
        m, rows = w.model, w.rows1
        x0, p0, _ = w.win1[0]
        inside = [x for x in range(x0 + 1, x0 + p0) if cb.judge(m, rows[x], rows[x - 1], 300, 25.0) == P]
        assert inside, "no MUM inside the run is passed against its list predecessor"
        own = cb.walk(m, rows, 300, 25.0, first=inside[0], back=inside[0] - 1)[0]
        assert own[:x0 + p0 + 1 - inside[0]] != w.v1[inside[0]:x0 + p0 + 1], "walked from inside, the run gives the same verdicts"
    if name == "reverse":
        m, rows = w.model, w.rows1
        rev = [bool(m.flags[r] & sc.ROW_REVERSE) for r in rows]
        assert any(rev[x] and w.v1[x] == P for x in range(len(rows))), "no passed MUM with a reverse-strand member"
        assert any(rev[x] and rev[w.b1[x]] and w.b1[x] < x - 1 for x in range(len(rows))), "no MUM with a reverse-strand member judged against a far back"
    if name == "second_pass":
        first = dict(zip(w.rows1, w.v1))
        second = dict(zip(w.rows, w.v2))
        assert w.info["lcbs_dissolved"] >= 1
        assert any(first[r] == P and second[r] == J for r in w.rows), "no MUM passed in the first pass joins in the second"
        assert any(first[r] == P and second[r] == P for r in w.rows), "no MUM stays passed"
        lens, last = [], None
        for r, v in zip(w.rows1, w.v1):
            if v == C_:
                lens.append(0)
            if v != P:
                lens[-1] += w.model.len[r]
        assert lens[-1] <= cb.CASES[name][4] and w.rows[-1] == w.rows1[-1], "the last LCB is not short, or did not stay"
    if name == "filler":
        assert w.fillers_over_passed >= 1, "no filler between two LCBs with a passed MUM in between"
    if name == "cap_8":
        assert w.info["trouble"] == 0 and w.info["lcbs_dissolved"] >= 1
    if name.startswith("second_pass_cap"):      # the run that meets the cap is the SECOND pass's: the dissolved LCB must still be in the layout
        assert max(p for _, p, _ in w.win1) == 5 and max(p for _, p, _ in w.win2) == 9 and w.info["lcbs_dissolved"] == 1, (w.win1, w.win2, w.info)
        assert (w.info["trouble"] == cb.WINDOW_BIT) == name.endswith("_8")
    if name == "cap_9":
        assert w.info["trouble"] == cb.WINDOW_BIT and w.info["lcbs_dissolved"] >= 1      # (what the restatement WOULD dissolve: the layout must not show it)


@pytest.mark.parametrize("name", sorted(cb.CASES))
def test_designed_list(lib, name):
    check_floors(name, cb.check_case(lib, name))


def test_the_default_mode_reports_nothing_passed(lib):
    """diag_diff <= 1: no head byte 2, pm_store_chain_passed (0, 0)"""
    n, items, d, _, c, _, _ = cb.CASES["runs123_join"]
    seqs = cb.build(7, n, items)
    with sc.Store(lib, seqs) as st:
        assert st.settle()[0] == sc.PM_OK
        m = sc.Model(seqs, st.raw_start, st.strand, st.lon, st.flags).settle()
        want = m.chain(d, 0.12, c)
        got, rows, heads = st.chain(len(m.acc_rows()), d, 0.12, c)
        assert got == want[0] and list(rows) == want[1] and list(heads) == want[2] and st.sess.chain_passed() == (0, 0)


def test_the_abi(lib, cpu_checkers):
    hdr = open(os.path.join(ROOT, "include", "parsnp_mum.h")).read()
    assert re.search(r"\bint pm_store_chain_passed\(const pm_session\* s, int64_t\* first_pass, int64_t\* second_pass\);", hdr) and '"chain_window"' in hdr
    syms = subprocess.run(["nm", "-D", "--defined-only", HIP_LIB], capture_output=True, check=True).stdout.decode()
    assert re.search(r" T pm_store_chain_passed$", syms, re.M)
    seqs = cb.build(7, 3, cb.CASES["pass_at_1"][1])
    with Session(lib, seqs) as s:
        with pytest.raises(PmError):
            s.chain_passed()      # (no chain call has ended)
        for bad in (0, 65537):
            with pytest.raises(PmError):
                s.tune("chain_window", bad)
        s.tune("chain_window", 65536)
    cpu = Lib(os.path.join(ROOT, "oracle", "_ref", "libpm_oracle.so"))      # a provider without the symbol
    with Session(cpu, seqs) as s, pytest.raises(PmError):
        s.chain_passed()


def test_sanitized_program(tmp_path):
    """tests/emu/chain_bp_check.cpp: runs of 1, 2, 3, 63, 64 and 65 passed MUMs, ended by a join and by a close, and a run of 8 and
    of 9 under a cap of 8, through the chain kernels in the emulation, as a program of its own under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "chain_bp_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPM_WAVE_EVENTS=5",
                    os.path.join(ROOT, "tests", "emu", "chain_bp_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "chain_bp_check ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------------------ end to end
E2E_SETS = {
    # name: (synth.make name, its overrides, ini keys).  Indels of several bases: the stock populations carry 1-base deletions only
    "indel6x120k_25": ("pop6x200k", dict(n=120_000, indel_frac=0.3, indel_len=40), dict(diagdiff=25)),
    "indel12x150k_25": ("pop12x400k", dict(n=150_000, indel_frac=0.3, indel_len=60), dict(diagdiff=25)),
    "indel6x120k_100bp": ("pop6x200k", dict(n=120_000, indel_frac=0.3, indel_len=150), dict(diagdiff="100bp")),
}


def e2e_inputs(name, base):
    made, override, kw = E2E_SETS[name]
    r, gs = synth.make(made, **override)
    return synth.write_set(os.path.join(base, "in"), r, gs) + (kw,)


def check_end_to_end(core, name, tmp, host_logic):
    """three steps in one process (PARSNP_STEPS, a test hook of the binary), the last one written"""
    want = json.load(open(GOLDEN))[name]
    assert want["chain_passed"] >= 10, "the set shows fewer than 10 passed MUMs in the first pass"
    rp, qs, kw = e2e_inputs(name, str(tmp))
    out = os.path.join(str(tmp), "out")
    log, timing = os.path.join(str(tmp), "route.log"), os.path.join(str(tmp), "timing.json")
    env = dict(os.environ, PARSNP_PARALLEL_MIN="8", PARSNP_FREE_MIN="2", PM_DIRTY_MIN="8", PARSNP_RESIDENT_LOG=log, PARSNP_CHECK_ZERO="1", PARSNP_STEPS="3")
    if host_logic:
        env["PARSNP_NO_DEVICE_CHAIN"] = "1"
    rc, _ = driver.run_core(core, rp, qs, out, timing=timing, env=env, threads=4, timeout=600, **kw)
    assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
    assert xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")) == want["xmfa_md5"]
    assert xmfa_util.log_counters(os.path.join(out, "parsnpAligner.log")) == want["log"]
    route = open(log).read().splitlines()
    assert len(route) == 3 and all("resident=1" in ln for ln in route), route
    assert all(("chain=1" in ln) == (not host_logic) for ln in route), route
    assert driver.read_timing(timing)["chain_passed"] == want["chain_passed"]


@pytest.mark.parametrize("host_logic", [False, True], ids=["device_chain", "host_list_logic"])
@pytest.mark.parametrize("name", sorted(E2E_SETS))
def test_end_to_end(emu, tmp_path, name, host_logic):
    check_end_to_end(emu[1], name, tmp_path, host_logic)
