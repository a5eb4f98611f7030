"""The suffix-array path of the event search on the device: the cases, checks and floors of tests/test_dense_edges.py (which runs them
in the kernel emulation) through libparsnp_hip.so.  Only here the radix sort of a doubling round is given a bit range
(`32 + bits_for(top_rank)`: the emulation's sort_pairs ignores it) -- test_sort_width holds the batches whose largest rank needs the
top bit of that range -- and only here the events of SeedDense arrive through the slices' atomics in an order of their own, so every
batch runs a second time in a fresh session and must give identical bytes.  pm_find_events opens a session per call (33 ms on the
MI355X), so a test makes at most about 100 such calls: (A), (B), (D) and (E) are one call per reference or go through sessions and stay
whole; of (C) the owner windows, the tail rule, the uniqueness and the N cases stay whole, the `order` and `left` families run two of
the four calls per (case, L) -- the query as planted on one strand and reverse-complemented on the other, which way round alternating
with the case's index + L -- and the catalogue of searchgen.py runs the (minsize, family) listed in CATALOGUE, every strand.  The
smallest cases come first, in a process of its own under a time limit: a kernel that does not come back fails that test, and every other test of the
file with it, before anything larger is launched.  Nothing here reads the reference tree."""
import os
import subprocess
import sys

import pytest

import densegen as G
import oracles
import test_dense_edges as T
from conftest import ROOT
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu

# (minsize, family) of test_search_edges.STREAM_CASES: every stride class with the edge lengths, the 40-base copy inside a long match
# (len == rep' and rep' + 1, shared K-mers) at every minimum length, arms from memory, the leaders, one set of clamps
CATALOGUE = [(8, "edges"), (17, "edges"), (31, "edges"), (48, "edges"), (19, "long"), (90, "long"), (25, "leaders"), (17, "clamps")] + \
            [(m, "repeats") for m in (8, 16, 17, 19, 25, 31, 32, 48, 90)]
THINNED = ("order", "left")


@pytest.fixture(scope="module")
def first(cpu_checkers):
    """`python tests/densegen.py first LIB`: rep' of references of 1, 2 and 3 bases and the one-round anchor call"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("PARSNP_TUNE", None)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "densegen.py"), "first", HIP_LIB], capture_output=True, text=True, env=env, timeout=120)
    except subprocess.TimeoutExpired as e:
        return "the smallest cases did not come back in 120 s: %s" % ((e.stdout or b"")[-500:],)
    if p.returncode != 0 or "first ok" not in p.stdout:
        return "exit code %d\n%s\n%s" % (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return None


@pytest.fixture(scope="module")
def libs(first, cpu_checkers):
    assert first is None, "the smallest cases failed (test_smallest_cases_first): nothing larger is launched\n" + first
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: there is no fall-back
    assert H.provider == "hip"
    return H, oracles.load_restatement()


def test_smallest_cases_first(first):
    assert first is None, first


@pytest.mark.parametrize("name", T.A_NAMES)
def test_rep_at_every_position(libs, name):
    T.check_rep(libs[0], libs[1], name)


@pytest.mark.parametrize("r", range(1, 10))
def test_rounds(libs, r):
    T.check_rounds(libs[0], libs[1], r)


@pytest.mark.parametrize("name", T.ROUND_BATCHES)
def test_rounds_of_a_batch(libs, name):
    T.check_round_batch(libs[0], libs[1], name, twice=True)


@pytest.mark.parametrize("family", G.PAIR_FAMILIES)
def test_seed_dense(libs, family):
    T.check_family(libs[0], libs[1], family, thin=family in THINNED)


def test_catalogue_selection():
    assert set(CATALOGUE) <= set(T.S.STREAM_CASES) and len(set(CATALOGUE)) == len(CATALOGUE)


@pytest.mark.parametrize("minsize,family", CATALOGUE)
def test_catalogue_on_this_path(libs, minsize, family):
    T.check_catalogue(libs[0], libs[1], minsize, family)


def test_queue_overflow(libs):
    T.check_overflow(libs[0], libs[1])


def test_segments(libs):
    T.check_segments(libs[0], libs[1], twice=True)


@pytest.mark.parametrize("nflag,n", G.WIDTHS)
def test_sort_width(libs, nflag, n):
    T.check_width(libs[0], libs[1], nflag, n, twice=True)


def test_budget_splits_a_batch(libs):
    T.check_budget(libs[0], libs[1], twice=True)


def test_calls_in_a_row(libs):
    T.check_calls_in_a_row(libs[0], libs[1])


def test_smaller_call_after_a_larger(libs):
    T.check_smaller_after_larger(libs[0], libs[1])
