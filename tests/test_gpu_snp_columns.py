"""pm_snp_* on the device: the cases and checks of tests/test_snp_columns.py (which runs them in the kernel emulation), through
libparsnp_hip.so.  Here the lanes of SnpClassify read a row's bytes side by side and count per wavefront, the ballots of SnpPack are
real, and SnpDist's tiles go through LDS on many wavefronts at once.  Then the writer of the product binary with snps=1."""
import numpy as np
import pytest

import snpcols as sn
import test_snp_columns as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_matrix(lib, name):
    T.check_case(lib, name)


def test_arguments(lib):
    T.check_arguments(lib)


def test_tall_matrix(lib):
    """640 rows (20 tiles a side, 210 of them computed) and 1 000 core SNPs (16 plane words: two full slabs) in three adds"""
    rng = np.random.default_rng(5)
    mats = [sn.matrix(sn.mixed(w, 640, rng, snps=k), 640, rng)[0] for w, k in ((500, 333), (1, 1), (900, 666))]
    exp = sn.expected(mats)
    assert exp[0]["core_snps"] == 1000
    with T.two_genomes(lib) as s:
        T.compare(s.core_snps(mats), exp, "tall")
        names = [n for n, _ in s.last_timing()]
    assert "snp_dist" in names


@pytest.mark.parametrize("variant", T.E2E_VARIANTS)
@pytest.mark.parametrize("name", list(T.E2E_SETS))
def test_files(tmp_path, name, variant):
    """the three files of a run of the product binary with snps=1 (the aligned gaps come from the device forms here)"""
    from parsnp_amd.paths import CORE_HOOKS_BIN
    T.check_e2e(CORE_HOOKS_BIN, name, variant, str(tmp_path), threads=8)
