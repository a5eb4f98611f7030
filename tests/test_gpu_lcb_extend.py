"""The LCB extension on the device: the designs and checks of tests/test_lcb_extend.py (which runs them in the kernel emulation),
through libparsnp_hip.so.  Here the table is walked by anti-diagonals with two cells a lane and one cross-lane move a step, the line
maxima gather in LDS, the two-bit moves of a pair lie in LDS while the first lane walks the path back, and the slot widths are a
maximum over the rows of a job.  Then the writer of the product binary with lcbext=1."""
import pytest

import test_lcb_extend as E
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("W,F,scores", E.TABLES)
def test_tables(lib, W, F, scores):
    E.check_tables(lib, W, F, scores)


@pytest.mark.parametrize("n", E.ROWS)
def test_rows(lib, n):
    E.check_rows(lib, n)


@pytest.mark.parametrize("n_jobs", [1, 2, 257])
def test_batches(lib, n_jobs):
    names = E.check_batches(lib, n_jobs)
    assert {"ext_reach", "ext_cut", "ext_trace", "ext_merge"} <= set(names)


def test_paths(lib):
    E.check_paths(lib)


def test_orientation(lib):
    E.check_orientation(lib)


def test_arguments(lib):
    E.check_arguments(lib)


def test_files(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    E.check_e2e(CORE_HOOKS_BIN, str(tmp_path), threads=8)


def test_limits(tmp_path):
    from parsnp_amd.paths import CORE_HOOKS_BIN
    E.check_limits(CORE_HOOKS_BIN, str(tmp_path))
