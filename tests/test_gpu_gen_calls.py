"""The generation calls of the resident route's recursion (pm_store_search / _search_beside, pm_store_validate, pm_store_order_check)
on the device, call by call against the sequential work list of tests/gencalls.py: the cases, checks and floors of
tests/test_gen_calls.py (which runs them in the kernel emulation), through libparsnp_hip.so.  Here the clusters of a call really
run side by side, one wavefront each, `lanes_for` hands lane t the genomes t, t + 64, ... (70 and 131 genomes wrap), the owner
arrays are filled by atomics and the children's slots go to whichever wavefront asks first -- which is why the children are compared
through their listed order and never by id.

The order of the wavefronts is the device's own, so instead of the emulation's reversed launches every case runs a second time in
a fresh session of the same process: done[], info[], the listed children and the layout of every call must be identical.

One process, one session open at a time, no subprocess; nothing here can fault the device: every list given to the engine is one
the former made from the engine's own regions, and the refused calls are refused on the host before anything is launched."""
import pytest

import gencalls as G
import test_gen_calls as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("case", list(G.CASES))
def test_floors(case):
    T.check_floors(case)


@pytest.mark.parametrize("case", list(G.CASES))
def test_generations(lib, case):
    T.check_generations(lib, case)


@pytest.mark.parametrize("case", list(G.CASES))
def test_second_session_is_identical(lib, case):
    first = T.run(lib, case)
    again = G.run_case(lib, case)
    assert len(again.trace) == len(first.trace)
    for i, (a, b) in enumerate(zip(again.trace, first.trace)):
        for what, x, y in zip(("done[]", "info[]", "the children", "the layout"), a, b):
            assert x == y, "%s: %s of call %d differs between two sessions" % (case, what, i)
    assert (again.trouble, again.order) == (first.trouble, first.order)


def test_end_state(lib):
    T.check_end_state(lib)


@pytest.mark.parametrize("case", list(G.CASES))
def test_one_cluster_per_generation(lib, case):
    T.check_coarse(lib, case)


def test_two_stages(lib):
    T.check_two_stages(lib)


@pytest.mark.parametrize("case", ["collinear70", "collinear131"])
def test_cluster_unsure(lib, case):
    T.check_cluster_unsure(lib, case)


def test_null_done(lib):
    T.check_null_done(lib)


def test_refusals_and_lists(lib):
    T.check_refusals_and_lists(lib)
