"""Bootstrap support of the SNP tree on the device: the designs and checks of tests/test_boot_support.py (which runs them in the
kernel emulation), through libparsnp_hip.so.  Here the draws are counted with atomic adds, the weight planes are ballots, the weight
words of SnpDistBoot sit in scalar registers, the trees of a batch share the launches of one tree with a workgroup per tree at the
barriers of NjJoin, and the splits are matched through the hash table in LDS.  Then the writer of the product binary with
bootstrap=B."""
import pytest

import test_boot_support as B
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("n,v,reps", B.SHAPES)
def test_generated_weights(lib, n, v, reps):
    B.check_generated(lib, n, v, reps)


@pytest.mark.parametrize("n,v,reps", [x for x in B.SHAPES if x[1]])
def test_caller_weights(lib, n, v, reps):
    B.check_caller_weights(lib, n, v, reps)


def test_batches(lib):
    B.check_batches(lib)


def test_arguments(lib):
    B.check_arguments(lib)


@pytest.mark.parametrize("name", B.BATCH_NAMES)
def test_trees(lib, name):
    B.check_trees(lib, name)


def test_limit(lib):
    """two trees of 2 048 leaves in lock step: the launches of one"""
    assert "boot_nj" in B.check_limit(lib)


@pytest.mark.parametrize("n", B.SUPPORT_ROWS)
def test_support(lib, n):
    B.check_support(lib, n)


def test_support_limit(lib):
    B.check_support_limit(lib)


@pytest.mark.parametrize("name", list(B.bs.CHAIN_DESIGNS))
def test_chain(lib, name):
    assert "boot_support" in B.check_chain(lib, name)


def test_files(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    B.check_e2e(CORE_HOOKS_BIN, str(tmp_path), threads=8)


def test_few_and_too_many(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    B.check_few_and_too_many(CORE_HOOKS_BIN, str(tmp_path), threads=8)
