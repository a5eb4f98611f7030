"""GroupedPairEventsWide on the device: the designed batches, checks and counts of tests/test_grouped_wide.py (which runs them in the
kernel emulation) through libparsnp_hip.so -- the election over LDS, the lanes' shares of the (piece, strand) tasks and their
diagonals, the 46 KB of tables per wavefront and the block counter shared with the first form, none of which the emulation
executes.  The smallest batches come first, in a process of their own under a time limit: a kernel that does not come back fails
that test, and every other test of the file with it, before anything larger is launched."""
import os
import subprocess
import sys

import pytest

import groupedwide as G
import oracles
import test_grouped_wide as T
from conftest import ROOT
from parsnp_amd.binding import Lib
from parsnp_amd.paths import CORE_HOOKS_BIN, HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def first(cpu_checkers):
    """`python tests/groupedwide.py first LIB`: 5 genomes (the wide launch finds every region done), then 40 genomes with 33 pieces, each with and without the wide form"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "groupedwide.py"), "first", HIP_LIB], capture_output=True, text=True, env=env, timeout=120)
    except subprocess.TimeoutExpired as e:
        return "the smallest batches did not come back in 120 s: %s" % ((e.stdout or b"")[-500:],)
    if p.returncode != 0 or "first ok" not in p.stdout:
        return "exit code %d\n%s\n%s" % (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout)
    return None


@pytest.fixture(scope="module")
def libs(first, cpu_checkers):
    assert first is None, "the smallest batches failed (test_smallest_batches_first): nothing larger is launched\n" + first
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: there is no fall-back
    assert H.provider == "hip"
    return H, oracles.load_restatement()


def test_smallest_batches_first(first):
    assert first is None, first


def test_group_limits(libs):
    T.check_limits(libs[0])


@pytest.mark.parametrize("n", T.PIECE_CASES)
def test_piece_boundaries(libs, n):
    T.check_pieces(libs[0], libs[1], n)


def test_event_lists(libs):
    T.check_events(*libs)


@pytest.mark.parametrize("nq,n", T.GENOME_CASES)
def test_genome_counts(libs, nq, n):
    T.check_genomes(libs[0], libs[1], nq, n)


@pytest.mark.parametrize("what", T.DEGENERATE_CASES)
def test_degenerate_regions(libs, what):
    T.check_degenerate(libs[0], libs[1], what)


def test_sharded_block(libs):
    T.check_sharded(*libs)


@pytest.mark.parametrize("name,wide", T.WHOLE_RUNS)
def test_whole_run(libs, tmp_path, name, wide):
    T.check_whole_run(CORE_HOOKS_BIN, name, wide, tmp_path, threads=8)
