"""pm_nj_tree on the device: the cases and checks of tests/test_nj_tree.py (which runs them in the kernel emulation), through
libparsnp_hip.so.  Here the butterflies of NjRowMin and NjJoin are real shuffles, the four wavefronts of NjJoin's workgroup meet at
its barriers, and the 2 (n - 3) + 2 launches of a tree are queued on the session's stream without a wait in between.  Then the
writer of the product binary with tree=1."""
import pytest

import test_nj_tree as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_tree(lib, name):
    T.check_case(lib, name)


def test_limit(lib):
    """2 048 leaves: about 4 100 short launches, one download"""
    assert "nj" in T.check_limit(lib)


def test_errors(lib):
    T.check_errors(lib)


def test_session_distances(lib):
    T.check_session_distances(lib)


def test_files(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    T.check_e2e(CORE_HOOKS_BIN, "pop6x200k", str(tmp_path), threads=8)


def test_names_and_two_sequences(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    T.check_names_and_two(CORE_HOOKS_BIN, str(tmp_path), threads=8)
