"""The suffix-array path of the event search (dense_kernels.h) on a real MI355X: the engine-level checks of
tests/test_dense_repeats.py against the HIP library, parsnp_core_hooks with every region on the path (PM_DENSE_ALL=1) against
the committed end-to-end goldens -- a 5 Mb anchor region and whole recursion batches through the device suffix array -- and
the tandem-array sets against the reference binary's recorded results, the last one at the shipped budget."""
import json
import os

import numpy as np
import pytest

import oracles
import test_dense_repeats as D
import test_host_logic
import xmfa_util
from parsnp_amd import driver, synth
from parsnp_amd.binding import Lib, Session
from parsnp_amd.paths import CORE_BIN, CORE_HOOKS_BIN, HIP_LIB
from test_golden import G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs(cpu_checkers):
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: no fallback
    assert H.provider == "hip"
    return H, oracles.load_restatement()


@pytest.mark.parametrize("minsize", [12, 20, 8])
def test_tandem_arrays_exceeding_the_budget(libs, minsize):
    D.test_tandem_arrays_exceeding_the_budget(libs, minsize)


def test_recursion_batch_with_one_dense_region(libs):
    D.test_recursion_batch_with_one_dense_region(libs)


def test_dense_all_against_walks_and_restatement(libs):
    H, O = libs
    assert D.dense_all_cases(H, O, np.random.default_rng(19), 200, 90) > 200


def test_dense_all_longer_regions(libs):
    D.test_dense_all_longer_regions(libs)


def test_mumi_coverage_on_a_tandem_array(libs):
    D.test_mumi_coverage_on_a_tandem_array(libs)


def test_dense_then_normal_then_dense(libs):
    D.test_dense_then_normal_then_dense(libs)


def test_dense_phases_in_the_timing(libs):
    """the device phases of the path appear on the calls that took it, and only there"""
    H, _ = libs
    rng = np.random.default_rng(8)
    ref = D.random_seq(rng, 2000) + D.UNIT * 700 + D.random_seq(rng, 2000)
    qs = [D.mutate(rng, ref, sub=0.01)]
    with Session(H, [ref] + qs) as s:
        s.whole(14)
        t = dict(s.last_timing())
        assert not [k for k in t if k.startswith("dense")], t
        s.tune("work_budget", 48)
        s.whole(14)
        t = dict(s.last_timing())
        assert t["dense_regions"] == 1 and t["dense_rounds"] >= 1 and "dense_overrun" in t, t
        assert "dense_sa" in t and "dense_search" in t, t
        s.tune("dense_all", 1)
        s.whole(14)
        t = dict(s.last_timing())
        assert t["dense_regions"] == 1 and "dense_sa" in t and "dense_overrun" not in t, t


E2E = json.load(open(os.path.join(G, "e2e.json")))


def check_e2e(name, rp, qs, kw, tmp_path, route):
    env = dict(os.environ, PM_DENSE_ALL="1", PARSNP_TIMING=str(tmp_path / "timing.json"))
    if route == "host":
        env["PARSNP_NO_RESIDENT"] = "1"
    out = str(tmp_path / "out")
    rc, _ = driver.run_core(CORE_HOOKS_BIN, rp, qs, out, env=env, threads=8, **kw)
    assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
    assert xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")) == E2E[name]["xmfa_md5"]
    assert xmfa_util.log_counters(os.path.join(out, "parsnpAligner.log")) == E2E[name]["log"]
    assert json.load(open(str(tmp_path / "timing.json")))["dense_regions"] >= 1


@pytest.mark.parametrize("route", ["resident", "host"])
@pytest.mark.parametrize("name", sorted(E2E))
def test_every_region_on_the_path_e2e(libs, tmp_path, name, route):
    """PM_DENSE_ALL=1: every region of every search takes the suffix-array path -- the committed goldens' bytes and counters"""
    if name == "mers":
        from test_golden import mers
        rp, qs = mers(base=str(tmp_path)); kw = {}
    else:
        rp, qs, kw = test_host_logic.harsh_inputs(name, str(tmp_path))
    check_e2e(name, rp, qs, kw, tmp_path, route)


@pytest.mark.parametrize("route", ["resident", "host"])
def test_every_region_on_the_path_bact200(tmp_path, route):
    """the 5 Mb anchor region of 200 bacterial genomes and the recursion batches after it, all on the device suffix array"""
    big = json.load(open(os.path.join(G, "e2e_big.json")))
    if "bact200" not in big:
        pytest.skip("no golden for bact200")
    ref, gs = synth.make("bact200")
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    env = dict(os.environ, PM_DENSE_ALL="1", PARSNP_TIMING=str(tmp_path / "timing.json"), OMP_WAIT_POLICY="passive")
    if route == "host":
        env["PARSNP_NO_RESIDENT"] = "1"
    out = str(tmp_path / "out")
    rc, _ = driver.run_core(CORE_HOOKS_BIN, rp, qs, out, env=env, threads=16, timeout=900)
    assert rc == 0, open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]
    assert xmfa_util.log_counters(os.path.join(out, "parsnpAligner.log")) == big["bact200"]["log"]
    assert xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")) == big["bact200"]["xmfa_md5"]
    assert json.load(open(str(tmp_path / "timing.json")))["dense_regions"] >= 1


@pytest.mark.parametrize("name", sorted(D.DENSE_SETS))
@pytest.mark.parametrize("route", ["host", "resident"])
def test_whole_runs_small_budget_on_gpu(tmp_path, monkeypatch, name, route):
    D.whole_run(CORE_HOOKS_BIN, name, tmp_path, monkeypatch, route)


# 4 genomes of 300 kb with a 10 000-copy array of a 7-base unit: RepeatLength compares a position of the array with ~10^4 chain
# entries of ~2 steps each, which exceeds the shipped budget of 2^22 steps
BIG_SET = dict(seed=90, n=300_000, ng=4, copies=10_000, spread=3)


def test_shipped_binary_default_budget(tmp_path):
    """the shipped parsnp_core at its default budget on a set whose tandem array exceeds it: the reference binary's bytes, and the
    run says that a region took the suffix-array path"""
    import refruns
    ref, gs = D.tandem_population(**BIG_SET)
    rp, qs = synth.write_set(str(tmp_path / "in"), ref, gs)
    kw = dict(threads=8)
    want = refruns.recorded(D.DENSE_GOLDEN, refruns.case_key(D.run_core, rp, qs, kw), refruns.REFBIN,
                            lambda: D.run_core(refruns.REFBIN, rp, qs, str(tmp_path / "ref"), kw))
    out = str(tmp_path / "mine")
    rc, _ = driver.run_core(CORE_BIN, rp, qs, out, timing=str(tmp_path / "timing.json"), timeout=900, **kw)
    got = refruns.normal((rc, xmfa_util.md5(os.path.join(out, "parsnpAligner.xmfa")) if rc == 0 else None,
                          xmfa_util.log_counters(os.path.join(out, "parsnpAligner.log")) if rc == 0 else open(os.path.join(out, "parsnp-aligner.err")).read()[-2000:]))
    assert got == want
    assert json.load(open(str(tmp_path / "timing.json")))["dense_regions"] >= 1
