"""The candidate side of a search call (pm_multi_mum_batch) on the device, row by row against the sequential restatement of
tests/candrows.py: the cases, checks and floors of tests/test_cand_rows.py (which runs them in the kernel emulation), through
libparsnp_hip.so.  Here the `__HIP_DEVICE_COMPILE__` bodies run: MasterEP's events staged in LDS 64 genomes at a time and its second walk
straight from memory above kEpCap entries (test_staging_overflow: more than 2 048 events of one chunk in the first 64-genome group, fewer
in the second), FoldCandidates' prefix minimum over the lanes with the carry between 64-genome groups, CandMark's ballot, a lane per
genome in DirtyExtent / DirtyPrefix / DirtyMark with their 8-row and 16-block rounds, clamped reads, ballots and an atomic OR per row,
and the grouped downloads of pm_copy_many (16-byte, 4-byte and byte-wise branches, tails, more than one 64 KB piece).

The order of the wavefronts is the device's own -- the atomic ORs of DirtyMark and the stores of CandWrite must not show -- so the cases
of the fold, of the overlap flags and of the carried capacities run a second time in a fresh session of the same process with identical
bytes.

One process, one session open at a time, no subprocess; every request row lies inside its genome.  Sharded sessions (StateAtCandidate,
PackStates / UnpackStates over uneven genome blocks) need two GPUs and concurrent ranks and are not covered here."""
import pytest

import candrows as R
import test_cand_rows as T
from parsnp_amd.binding import Lib
from parsnp_amd.paths import HIP_LIB

pytestmark = pytest.mark.gpu

FIELDS = ("off", "k", "lon", "start", "strand", "flags")


@pytest.fixture(scope="module")
def lib():
    lib = Lib(HIP_LIB)      # raises if the library is missing: there is no fall-back
    assert lib.provider == "hip"
    return lib


@pytest.mark.parametrize("family", T.FAMILIES)
def test_floors(family):
    T.check_floors(family)


@pytest.mark.parametrize("nq", R.FOLD_QUERIES)
def test_fold_at_group_edges(lib, nq):
    first = T.check_fold(lib, nq)
    again = T.check_fold(lib, nq)      # (fresh sessions)
    for a, b in zip(first, again):
        for x in ("off", "k", "lon", "sp", "fwd"):
            assert getattr(a, x).tobytes() == getattr(b, x).tobytes(), "fold %d: %s differs between two sessions" % (nq, x)


def test_candidate_counts(lib):
    T.check_counts(lib)


@pytest.mark.parametrize("starts,tail,late", T.CHUNK_CASES)
def test_chunk_edges(lib, starts, tail, late):
    T.check_chunks(lib, starts, tail, late)


def test_staging_overflow(lib):
    T.check_staging(lib)


def test_batch_listing(lib):
    T.check_batch(lib)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(R.FLAG_CASES))
def test_overlap_flags(lib, name, mode):
    first = T.check_flags(lib, name, mode)
    again = T.check_flags(lib, name, mode)      # (a fresh session)
    for x in FIELDS:
        assert getattr(first, x).tobytes() == getattr(again, x).tobytes(), "%s, rows %d: %s differs between two sessions" % (name, mode, x)
    assert (first.dirty_known, first.table_id != 0) == (again.dirty_known, again.table_id != 0)


def test_list_lengths_around_dirty_min(lib):
    T.check_list_lengths(lib)


def test_rows_of_four_and_five_bases(lib):
    T.check_short_rows(lib)


def test_capacities_carried_over(lib):
    assert T.check_capacities(lib) == T.check_capacities(lib), "rows or flags of the three anchor calls differ between two sessions"


@pytest.mark.parametrize("name", T.DOWNLOAD_CASES)
def test_downloads(lib, name):
    T.check_downloads(lib, name)
