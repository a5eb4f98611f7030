"""The suffix-array path of the event search (parsnp_amd/csrc/engine/dense_kernels.h) in the kernel emulation, against the CPU
restatement: regions whose K-mer chain walks exhaust the per-thread work budget -- tandem repeats of period > 1 with hundreds of
copies -- are flagged and run again on the suffix array instead of failing with PM_ELIMIT; tune "dense_all" puts every region
on it.  rep' of the path is checked here through the candidates (every event test compares ms with rep'[l0]).  pm_find_events runs
a session of its own, which PARSNP_TUNE=dense_all=1 puts on the path: tests/test_dense_edges.py compares rep' and the events of
SeedDense one by one that way."""
import ctypes as C
import os

import numpy as np
import pytest

import oracles
import refruns
import xmfa_util
from parsnp_amd import driver, synth
from parsnp_amd.binding import Lib, PmError, Session
from seqgen import adversarial_case, mutate, random_seq

UNIT = b"ACGTTGCA"      # period 8 (a palindrome as a whole: both strands of the array hit the same chains)
UNIT2 = b"AACGTGTC"
DENSE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_runs.json.xz")


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def tandem_sets(rng):
    """(name, ref, queries): arrays of 400 to 1 000 copies of an 8-base unit inside random flanks"""
    def flank(n):
        return random_seq(rng, n)
    c = int(rng.integers(400, 1001))
    arr = UNIT * c
    ref = flank(400) + arr + flank(500)
    yield "both", ref, [mutate(rng, ref, sub=0.01), flank(80) + UNIT * (c - 37) + flank(300)]
    yield "reference_only", ref, [flank(300) + ref[380:520] + flank(200) + ref[-450:], mutate(rng, flank(700), sub=0.0)]
    # (the reference keeps a short array: its chains exceed a budget of 48 steps as well, the query's long array hits them)
    short = flank(600) + UNIT2 * 30 + flank(600)
    yield "query_only", short, [flank(100) + UNIT2 * c + flank(100), mutate(rng, short, sub=0.02)]
    yield "reverse_in_query", ref, [oracles.revcomp(mutate(rng, ref, sub=0.01)), flank(100) + oracles.revcomp(UNIT * (c - 5)) + flank(100)]
    yield "region_edge", arr + flank(300), [mutate(rng, arr[:len(arr) // 2] + flank(300), sub=0.005), UNIT * (c + 3)]
    yield "two_units", flank(200) + UNIT * (c // 2) + flank(50) + UNIT2 * (c // 2) + flank(200), [UNIT * 40 + UNIT2 * (c // 3), flank(100)]


def timing(s):
    return dict(s.last_timing())


@pytest.mark.parametrize("minsize", [12, 20, 8])
def test_tandem_arrays_exceeding_the_budget(libs, minsize):
    """fails without the path: the 256x rerun (12 288 steps) runs out as well and the call returns PM_ELIMIT"""
    E, O = libs
    rng = np.random.default_rng(300 + minsize)
    for name, ref, qs in tandem_sets(rng):
        want = oracles.restatement_multi_mum(O, [ref] + qs, minsize, 1)
        with Session(E, [ref] + qs) as s:
            s.tune("work_budget", 48)
            got = s.whole(minsize)
            t = timing(s)
        assert same(want, got), (name, minsize)
        assert t.get("dense_regions", 0) >= 1, (name, t)
        assert t.get("budget_retries", 0) >= 1, (name, t)


def test_recursion_batch_with_one_dense_region(libs):
    """a batch shaped like the recursion's -- many small regions and a few longer ones -- with one region that holds a tandem
    array: that region alone takes the path, every other walks; the same candidates with the small regions grouped and not"""
    E, O = libs
    rng = np.random.default_rng(41)
    parts = [random_seq(rng, int(rng.integers(20, 400))) for _ in range(60)]
    dense_at = 17
    parts[dense_at] = random_seq(rng, 90) + UNIT * 500 + random_seq(rng, 90)
    ref = b"".join(parts)
    qs = [mutate(rng, ref, sub=0.02), mutate(rng, ref, sub=0.05)]
    starts, lens, ms = [], [], []
    at = 0
    for p in parts:
        starts.append([at, at, at]); lens.append([len(p)] * 3); ms.append(int(rng.integers(9, 21)))
        at += len(p)
    # pieces of the queries that are not the region's own bases in one of them
    starts[3][1] = starts[4][0]; starts[dense_at][2] = max(0, starts[dense_at][2] - 30)
    want = [oracles.restatement_multi_mum(O, [q[s:s + n] for q, s, n in zip([ref] + qs, st, ln)], m, 1) for st, ln, m in zip(starts, lens, ms)]
    for grp in (1, 0):
        with Session(E, [ref] + qs) as s:
            s.tune("work_budget", 48)
            s.tune("group_small", grp)
            got = s.multi_mum_batch(np.array(starts), np.array(lens), ms)
            t = timing(s)
        for r in range(len(parts)):
            assert same(want[r], got[r]), (grp, r)
        assert t.get("dense_regions") == 1, t


def dense_all_cases(E, O, rng, count, n_hi):
    total = 0
    for it in range(count):
        ref, qs = adversarial_case(rng, 10, n_hi, int(rng.integers(1, 4)))
        if it % 7 == 0:      # homopolymers and N runs
            ref = ref[: len(ref) // 2] + b"A" * int(rng.integers(5, 40)) + b"N" * int(rng.integers(1, 30)) + ref[len(ref) // 2:]
            qs[0] = qs[0] + b"A" * 30 + b"NNNN" + ref[-20:]
        if it % 11 == 0:     # palindromic K-mers
            pal = random_seq(rng, 6)
            ref = ref + pal + oracles.revcomp(pal) + ref[:10]
            qs[-1] = pal + oracles.revcomp(pal) + qs[-1]
        minsize = int(rng.integers(1, 24))      # K < minlen (stride > 1) from 17 on, K = minlen below
        want = oracles.restatement_multi_mum(O, [ref] + qs, minsize, 1)
        for d in (0, 1):
            with Session(E, [ref] + qs) as s:
                s.tune("dense_all", d)
                got = s.whole(minsize)
                t = timing(s)
            assert same(want, got), (it, d, minsize, ref, qs)
            if d and len(ref):
                assert t.get("dense_regions") == 1, t
            else:
                assert "dense_regions" not in t, t
        total += len(want[0])
    return total


def test_dense_all_against_walks_and_restatement(libs):
    E, O = libs
    assert dense_all_cases(E, O, np.random.default_rng(9), 300, 90) > 300


def test_dense_all_longer_regions(libs):
    """regions of thousands of positions: more doubling rounds, K-mers with stride > 1, windows that meet the piece's ends"""
    E, O = libs
    rng = np.random.default_rng(12)
    for it in range(12):
        ref = random_seq(rng, int(rng.integers(1500, 4000)))
        a = int(rng.integers(0, 800)); L = int(rng.integers(50, 600))
        ref = ref[:a + L] + ref[a:a + L] + ref[a + L:]          # a long exact repeat: rep' > 500
        qs = [mutate(rng, ref, sub=0.02, indel=0.002), oracles.revcomp(mutate(rng, ref[200:], sub=0.03))]
        minsize = int(rng.choice([9, 16, 21, 31]))
        want = oracles.restatement_multi_mum(O, [ref] + qs, minsize, 1)
        with Session(E, [ref] + qs) as s:
            s.tune("dense_all", 1)
            got = s.whole(minsize)
        assert same(want, got), (it, minsize)


def test_mumi_coverage_on_a_tandem_array(libs):
    """calcmumi (K = 15, stride 1) with a tiny budget: the pairwise coverage of the restatement"""
    E, O = libs
    O.oracle_mumi_coverage.restype = C.c_int64
    rng = np.random.default_rng(5)
    ref = random_seq(rng, 500) + UNIT * 600 + random_seq(rng, 700)
    qs = [mutate(rng, ref, sub=0.01), random_seq(rng, 200) + UNIT * 580 + ref[-600:], oracles.revcomp(ref)]
    want = [O.oracle_mumi_coverage(ref, C.c_int64(len(ref)), q, C.c_int64(len(q)), 1) for q in qs]
    with Session(E, [ref] + qs) as s:
        s.tune("work_budget", 16)
        got = s.mumi_coverage()
        t = timing(s)
    assert got == want
    assert t.get("dense_regions", 0) >= 1, t
    assert sum(want) > 1000


def test_dense_then_normal_then_dense(libs):
    """nothing of the path outlives its call: the same results each time, its timing keys only on the calls that took it"""
    E, O = libs
    rng = np.random.default_rng(3)
    ref = random_seq(rng, 300) + UNIT * 450 + random_seq(rng, 300)
    qs = [mutate(rng, ref, sub=0.01), random_seq(rng, 100) + UNIT * 420 + random_seq(rng, 100)]
    want_d = oracles.restatement_multi_mum(O, [ref] + qs, 11, 1)
    with Session(E, [ref] + qs) as s:
        s.tune("work_budget", 48)
        seen = []
        for step in range(3):
            got = s.whole(11)
            t = timing(s)
            assert same(want_d, got), step
            assert t.get("dense_regions", 0) >= 1 and "dense_overrun" in t, t
            seen.append(got)
            if step < 2:      # a batch without the array: the two flanks
                st = np.array([[0, 0, 0], [len(ref) - 300, len(qs[0]) - 300, 0]], np.int64)
                ln = np.array([[300, 300, 90], [300, 300, 90]], np.int64)
                got2 = s.multi_mum_batch(st, ln, [11, 11])
                t2 = timing(s)
                assert not [k for k in t2 if k.startswith("dense")], t2
                for r in range(2):
                    w = oracles.restatement_multi_mum(O, [x[a:a + n] for x, a, n in zip([ref] + qs, st[r], ln[r])], 11, 1)
                    assert same(w, got2[r]), (step, r)
    assert all(same(seen[0], x) for x in seen[1:])


def test_unknown_key_still_rejected(libs):
    E, _ = libs
    with Session(E, [b"ACGT" * 10, b"ACGT" * 10]) as s:
        s.tune("dense_all", 1)
        s.tune("dense_all", 0)
        with pytest.raises(PmError):
            s.tune("dense_everything", 1)


# ---------------------------------------------------------------------------------------------------------------- whole runs
def tandem_population(seed, n, ng, copies, unit=b"ACGGTCA", spread=6):
    """a small population whose genomes carry one tandem array of `copies` units at the same place (a few copies more or less)"""
    rng = np.random.default_rng(seed)
    ref, gs = synth.population(seed=seed, n=n, n_genomes=ng, div=0.01, indel_frac=0.05)
    at = n // 3

    def put(g, c):
        p = min(at, len(g) - 1)
        return g[:p] + unit * c + g[p:]
    ref = put(ref, copies)
    gs = [put(g, copies + int(rng.integers(-spread, spread + 1))) for g in gs]
    return ref, gs


DENSE_SETS = {
    "t7x1500": dict(seed=71, n=30_000, ng=4, copies=1500),
    "t7x800": dict(seed=72, n=60_000, ng=3, copies=800, unit=b"ACGTTCA"),
}


def run_core(core, rp, qs, out, kw):
    rc, _ = driver.run_core(core, rp, qs, out, timeout=900, **kw)
    x = os.path.join(out, "parsnpAligner.xmfa")
    lg = os.path.join(out, "parsnpAligner.log")
    return (rc, xmfa_util.md5(x) if os.path.exists(x) else None, xmfa_util.log_counters(lg) if os.path.exists(x) else open(lg).read())


def whole_run(core, name, tmp_path, monkeypatch, route, budget="64", world=1):
    ref, gs = tandem_population(**DENSE_SETS[name])
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    kw = dict(threads=3)
    want = refruns.recorded(DENSE_GOLDEN, refruns.case_key(run_core, rp, qs, kw), refruns.REFBIN,
                            lambda: run_core(refruns.REFBIN, rp, qs, str(tmp_path / "ref"), kw))
    monkeypatch.setenv("PM_WORK_BUDGET", budget)
    monkeypatch.setenv("PARSNP_TIMING", str(tmp_path / "timing.json"))
    if route == "resident":
        for k, v in dict(PM_DIRTY_MIN="2", PARSNP_PARALLEL_MIN="2", PARSNP_FREE_MIN="1").items():
            monkeypatch.setenv(k, v)
    else:
        monkeypatch.setenv("PARSNP_NO_RESIDENT", "1")
    if world == 1:
        got = refruns.normal(run_core(core, rp, qs, str(tmp_path / "mine"), kw))
        assert got == want, (name, route)
    return want, rp, qs, kw


@pytest.mark.parametrize("name", sorted(DENSE_SETS))
@pytest.mark.parametrize("route", ["host", "resident"])
def test_whole_runs_small_budget(emu, tmp_path, monkeypatch, name, route):
    """parsnp_core over the kernel emulation with a budget small enough that the anchor region's tandem array exceeds it: the
    reference binary's XMFA bytes and log counters"""
    whole_run(emu[1], name, tmp_path, monkeypatch, route)


def test_whole_run_sharded_gloo(emu, tmp_path, monkeypatch):
    """two ranks on gloo over the kernel emulation, the same small budget: each rank flags what its own walks exceeded, the
    decision to run the batch again travels with the first exchange -- the reference binary's bytes"""
    import subprocess
    import sys
    want, rp, qs, kw = whole_run(emu[1], "t7x1500", tmp_path, monkeypatch, "host", world=2)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "sharded")
    os.makedirs(out)
    ini = os.path.join(out, "run.ini")
    open(ini, "w").write(driver.ini_text(rp, qs, out, **kw))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PARSNP_CORE_LIB=os.path.join(root, "tests", "emu", "libparsnp_core_emu.so"), PYTHONPATH=root)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29573", "-m", "parsnp_amd.sharded", ini]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=out, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    x = os.path.join(out, "parsnpAligner.xmfa")
    assert [0, xmfa_util.md5(x), xmfa_util.log_counters(os.path.join(out, "parsnpAligner.log"))] == want
