"""pm_store_unalign_count / pm_store_unalign_runs on the device: the cases, checks and floors of tests/test_unalign_runs.py (which runs
them in the kernel emulation), through libparsnp_hip.so.  Here a wavefront's lanes take the 64 words of a block side by side, the
neighbour words travel through LDS, the counts of the blocks are scanned by rocPRIM and the lanes of many wavefronts store their
runs at once."""
import pytest

import test_unalign_runs as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("case", list(T.CASES))
def test_runs(lib, case):
    T.check_runs(lib, case)


def test_wrong_size_is_refused(lib):
    T.check_wrong_size(lib)


@pytest.mark.parametrize("route", ["resident", "host"])
@pytest.mark.parametrize("name", list(T.E2E_SETS))
def test_parsnp_unalign(tmp_path, name, route):
    """parsnp.unalign of whole runs on the device, both routes: the bytes of the bit-by-bit walk and of the reference, and on the
    resident route less than a layout image downloaded for it"""
    from parsnp_amd.paths import CORE_HOOKS_BIN
    T.check_e2e(CORE_HOOKS_BIN, name, route, str(tmp_path), threads=8)
