"""The DEVICE bodies of the kernels between the event search and the fold (EventPlace's returning add per run, CoarseFromBuckets'
tiles through LDS, WaveSummary's butterfly, SummaryCarry's segmented scan and reduction, WaveScan's rounds behind its carry) on the
designed inputs of tests/test_event_scan_edges.py, through libparsnp_hip.so: the same cases, checks and floors, the carries at the
size of the device's wavefronts (512 events; a chunk of SummaryCarry is 8 192)."""
import pytest

import oracles
import searchgen as G
import test_event_scan_edges as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs(cpu_checkers):
    H = Lib(HIP_LIB)          # raises if the HIP library is missing: there is no fall-back
    assert H.provider == "hip"
    return H, oracles.load_restatement()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_runs_inside_a_lane(libs, which):
    T.check_runs(libs[0], libs[1], which)


def test_carries_across_chunks(libs):
    T.check_carries(libs[0], libs[1], G.WAVE_EVENTS, count_every_pair=False)


def test_every_wavefront_opens_a_pair(libs):
    T.check_no_carry(libs[0], libs[1], G.WAVE_EVENTS)


@pytest.mark.parametrize("n,nq", T.COARSE_CASES)
def test_coarse_table(libs, n, nq):
    T.check_coarse(libs[0], libs[1], n, nq)


@pytest.mark.parametrize("nq,long_every,floor", [(5, 0, 20), (70, 0, 5), (9, 11, 20)])      # (70 genomes at 3 % divergence share few stretches)
def test_one_block_regions(libs, nq, long_every, floor):
    assert T.check_one_block_batch(libs[0], libs[1], 40 + nq, nq, 300 if nq < 20 else 120, long_every) > floor


@pytest.mark.parametrize("name", ["empty_ends", "long_bucket", "last_bucket"])
def test_cursors(libs, name):
    T.check_cursors(libs[0], libs[1], name)
