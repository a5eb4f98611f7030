"""The recombination scan of the core SNP columns on the device: the designs and checks of tests/test_rec_phi.py (which runs them in
the kernel emulation), through libparsnp_hip.so.  Here the transposed planes are ballots, the letter sets of a pair of sites meet in
registers with their row words staged through LDS, and a window's matrix lies in LDS while a wavefront ranks the keys of one
permutation after the other.  Then the writer of the product binary with recomb=1."""
import pytest

import test_rec_phi as R
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("n,v", R.SHAPES)
def test_sites(lib, n, v):
    R.check_sites(lib, n, v)


def test_rows2048(lib):
    R.check_rows2048(lib)


def test_adds(lib):
    R.check_adds(lib)


def test_pairs(lib):
    R.check_pairs(lib)


@pytest.mark.parametrize("k", R.K_SIZES)
def test_windows(lib, k):
    R.check_windows(lib, k)


def test_batches(lib):
    names = R.check_batches(lib)
    assert {"rec_sites", "rec_incompat", "rec_permute"} <= set(names)


def test_designed(lib):
    R.check_designed(lib)


def test_arguments(lib):
    R.check_arguments(lib)


def test_files(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    R.check_e2e(CORE_HOOKS_BIN, str(tmp_path), threads=8)


def test_few_and_limits(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    R.check_few_and_limits(CORE_HOOKS_BIN, str(tmp_path), threads=8)
