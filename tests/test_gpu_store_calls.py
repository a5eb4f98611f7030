"""The entry points of the resident route (include/parsnp_mum.h: pm_store_*) on the device, call by call against the sequential
restatement of tests/storecalls.py: the cases, checks and floors of tests/test_store_calls.py (which runs them in the kernel
emulation), through libparsnp_hip.so.  Here `lanes_for` hands lane t the genomes t, t + 64, ..., the reductions run over the
wavefront, the marks are atomics and L2-coherent loads, and the rows of a case are settled by many wavefronts at once."""
import pytest

import test_store_calls as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu
CASES = [c for c in T.CASES if c not in T.REVERSED]      # (the order of the wavefronts is the device's own)


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("case", CASES)
def test_settle(lib, case):
    T.check_settle(lib, case)


@pytest.mark.parametrize("case", CASES)
def test_layout(lib, case):
    T.check_layout(lib, case)


@pytest.mark.parametrize("case", CASES)
def test_rows(lib, case):
    T.check_rows(lib, case)


@pytest.mark.parametrize("case", CASES)
def test_judge(lib, case):
    T.check_judge(lib, case)


@pytest.mark.parametrize("case", CASES)
def test_fill(lib, case):
    """add == 2 cannot be reached with valid rows (a chain end at a genome's end makes the overlap test, which comes first, answer 0:
    derived in check_fill's docstring), so the cases hold add == 0 and add == 1 only and assert that neither side reports 2"""
    T.check_fill(lib, case)


@pytest.mark.parametrize("case", CASES)
def test_unmark(lib, case):
    T.check_unmark(lib, case)


@pytest.mark.parametrize("case", CASES)
def test_settle_seeds(lib, case):
    T.check_settle_seeds(lib, case)


@pytest.mark.parametrize("case", T.CHAIN_CASES)
def test_chain(lib, case):
    T.check_chain(lib, case)
