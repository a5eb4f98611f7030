"""Phases C-D for a diagonal difference given in bases on the device: the designed lists, checks and floors of
tests/test_chain_bp.py (which runs them in the kernel emulation) through libparsnp_hip.so -- the reductions over the lanes in
ChainWindow, the strided writes of ChainWindowFill and the order of the launches on one queue, none of which the emulation
executes -- and the end-to-end sets through parsnp_core_hooks.  The smallest list comes first, in a process of its own under a
time limit: a kernel that does not come back fails that test, and every other test of the file with it, before anything larger
is launched."""
import os
import subprocess
import sys

import pytest

import chainbp as cb
import test_chain_bp as T
from conftest import ROOT
from parsnp_amd.binding import Lib
from parsnp_amd.paths import CORE_HOOKS_BIN, HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def first():
    """`python tests/chainbp.py first LIB`: 9 MUMs in 3 genomes, the second of them passed"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chainbp.py"), "first", HIP_LIB], capture_output=True, text=True, env=env, timeout=120)
    except subprocess.TimeoutExpired as e:
        return "the smallest list did not come back in 120 s: %s" % ((e.stdout or b"")[-500:],)
    if p.returncode != 0 or "first ok" not in p.stdout:
        return "exit code %d\n%s\n%s" % (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return None


@pytest.fixture(scope="module")
def lib(first):
    assert first is None, "the smallest list failed (test_smallest_list_first): nothing larger is launched\n" + first
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: there is no fall-back
    assert H.provider == "hip"
    return H


def test_smallest_list_first(first):
    assert first is None, first


@pytest.mark.parametrize("name", sorted(cb.CASES))
def test_designed_list(lib, name):
    T.check_floors(name, cb.check_case(lib, name))


def test_the_default_mode_reports_nothing_passed(lib):
    T.test_the_default_mode_reports_nothing_passed(lib)


@pytest.mark.parametrize("host_logic", [False, True], ids=["device_chain", "host_list_logic"])
@pytest.mark.parametrize("name", sorted(T.E2E_SETS))
def test_end_to_end(lib, tmp_path, name, host_logic):
    T.check_end_to_end(CORE_HOOKS_BIN, name, tmp_path, host_logic)
