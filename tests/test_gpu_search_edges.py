"""The DEVICE bodies of the event search (parsnp_amd/csrc/engine/kernels.h) on the designed pairs of tests/searchgen.py: the cases,
checks and floors of tests/test_search_edges.py (which runs them in the kernel emulation, through the sequential `#else` twins)
through libparsnp_hip.so.  Here the leaders' hits travel by __shfl (`before` / `after` at g0 == 0 and g0 == 64 - kLead), the arms
end by the segmented suffix minimum over the lanes, an arm that outruns its wavefront is finished by the whole wavefront 64 * 32
bases a round, the bucket counters are added run by run (__shfl_up heads, __ballot run lengths), and the scan is the 64-lane
segmented pair_scan with the carry across 512 events -- none of which the emulation executes.  Also the device twins of what ran
in the emulation only: test_long_minimum_lengths, and test_events' adversarial inputs at a size that is no small_pair."""
import pytest

import oracles
import searchgen as G
import test_emu_engine
import test_search_edges as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu
TUNES = ({}, {"bucket_sort": 0}, {"master_seg": 0}, {"bucket_sort": 0, "master_seg": 0})


@pytest.fixture(scope="module")
def libs(cpu_checkers):
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: there is no fall-back
    assert H.provider == "hip"
    return H, oracles.load_restatement()


@pytest.mark.parametrize("minsize,family", T.STREAM_CASES)
def test_event_streams(libs, minsize, family):
    T.FAMILIES[family](libs[0], libs[1], minsize)


def test_bucket_populations(libs):
    T.check_buckets(libs[0], libs[1], TUNES)


@pytest.mark.parametrize("which", [0, 1])
def test_scan_carry(libs, which):
    T.check_scan(libs[0], libs[1], which, TUNES)


def test_equal_reach(libs):
    T.check_ties(libs[0], libs[1], TUNES)


def test_events_beyond_small_pairs(libs):
    T.check_adversarial_events(libs[0], libs[1], 120, 18)


def test_long_minimum_lengths(libs):
    """minsize 48 .. 130 on the device: no `regs`, the tags from memory, every sample probes for itself, both arms from memory"""
    test_emu_engine.test_long_minimum_lengths(libs)
