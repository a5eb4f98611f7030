"""The small-region event search on the device: the cases, checks and floors of tests/test_small_pairs.py (which runs them in the
kernel emulation) through libparsnp_hip.so -- SmallPairEvents with wave_reserve01 and the slices' atomics, the LDS tables of
GroupedPairEvents and GroupedPairEventsWide between their wave_syncs, the lanes' shares of a task's diagonals, none of which the
emulation executes.  pm_find_events opens a session per call (33 ms on the MI355X), so the corner stretches are thinned to four (case, L)
combinations a pair of lengths and the whole shorter side at L == its length, each with two of the four calls (every pair of
lengths stays; the places, the kinds of L and the strand that reads the planted bases rotate from pair to pair; the emulation runs
them all), and the bulk goes through the batches, one session per batch and route.  Every batch runs a second time in fresh
sessions and must give identical bytes (the order of the atomics).  The smallest batch comes first, in a process of its own under
a time limit: a kernel that does not come back fails that test, and every other test of the file with it, before anything larger
is launched."""
import os
import subprocess
import sys

import pytest

import oracles
import smallgen as G
import test_small_pairs as T
from conftest import ROOT
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def first(cpu_checkers):
    """`python tests/smallgen.py first LIB`: the batch of the packed fields (4 query genomes, 9 regions) through the three routes"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "smallgen.py"), "first", HIP_LIB], capture_output=True, text=True, env=env, timeout=120)
    except subprocess.TimeoutExpired as e:
        return "the smallest batch did not come back in 120 s: %s" % ((e.stdout or b"")[-500:],)
    if p.returncode != 0 or "first ok" not in p.stdout:
        return "exit code %d\n%s\n%s" % (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout)
    return None


@pytest.fixture(scope="module")
def libs(first, cpu_checkers):
    assert first is None, "the smallest batch failed (test_smallest_batch_first): nothing larger is launched\n" + first
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: there is no fall-back
    assert H.provider == "hip"
    return H, oracles.load_restatement()


def test_smallest_batch_first(first):
    assert first is None, first


@pytest.mark.parametrize("nR", G.LENGTHS + (129,))
def test_corner_stretches(libs, nR):
    T.check_corners(libs[0], libs[1], nR, thin=True)


@pytest.mark.parametrize("family", T.FAMILIES)
def test_special_pairs(libs, family):
    T.check_special(libs[0], libs[1], family)


def test_ends_batch(libs):
    T.check_ends(libs[0], libs[1], twice=True)


def test_fields_batch(libs):
    T.check_fields(libs[0], libs[1], twice=True)


@pytest.mark.parametrize("nq", [70, 130])
def test_lanes_batch(libs, nq):
    T.check_lanes(libs[0], libs[1], nq, twice=True)


def test_tandem_batch(libs):
    T.check_tandem(libs[0], libs[1], twice=True)
