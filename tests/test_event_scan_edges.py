"""What happens to the events between the search and the fold (parsnp_amd/csrc/engine/kernels.h: EventPlace on its cursors,
CoarseFromBuckets by tiles, WaveSummary as a reduction, SummaryCarry, WaveScan with its carry from there) on inputs DESIGNED
for the edges of those kernels, against the CPU restatement.  This module runs the cases in the kernel emulation (the sequential
`#else` twins, wavefronts of 5 events) and tests/test_gpu_event_scan_edges.py runs them through libparsnp_hip.so, at the sizes of
the device's wavefronts.

  RUN          8: pairs of RUN, RUN + 1, 64 RUN - 1, 64 RUN, 64 RUN + 1 events put a pair's first event on the first and the last lane
               of a round of WaveScan, on lanes in between, and on a wavefront's first event (and on the first, a middle and the last
               event of a run of RUN events per lane, the form of WaveScan that was measured and not kept: profiles/event_scan); the
               batches end in a last wavefront of 1, RUN - 1 and RUN + 1 events
  CARRY_TILES  wavefronts per wavefront of SummaryCarry (kCarryTiles): a pair over more than two chunks of them, between pairs that
               end with a chunk; a batch in which every wavefront opens a pair
  COARSE_ROWS, COARSE_GEN   the tile of CoarseFromBuckets: 1, 63, 64, 65 and 200 query genomes; regions of 255, 256, 257 and
               64 * 256 + 1 positions; batches of one-block regions, grouped and not
Every case asserts floors from the restatement's output (the pairs hold the designed numbers of events), so that a generator which
stops reaching an edge turns the test red."""
import functools
import os
import re

import numpy as np
import pytest

import oracles
import searchgen as G
import test_search_edges as T
from parsnp_amd.binding import Lib, Session
from seqgen import mutate, random_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = 8
CARRY_TILES = 16    # kCarryTiles
COARSE_ROWS, COARSE_GEN = 32, 64      # kCoarseRows, kCoarseGen
EMU_WAVE = 5        # events per wavefront of the emulation's build (tests/conftest.py: -DPM_WAVE_EVENTS=5)
TUNES = ({}, {"bucket_sort": 0})


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "parsnp_amd", "csrc", "engine", "kernels.h")).read()
    assert int(re.search(r"constexpr int kCarryTiles = (\d+);", src).group(1)) == CARRY_TILES
    assert re.search(r"constexpr int kCoarseRows = (\d+), kCoarseGen = (\d+);", src).groups() == (str(COARSE_ROWS), str(COARSE_GEN))
    assert G.WAVE_EVENTS == 64 * RUN      # (the batches below are designed for wavefronts of 64 runs)


# ------------------------------------------------------------------------------------------ runs inside a lane
W = G.WAVE_EVENTS
RUN_COUNTS = ((W - 1, RUN, RUN + 1, W, W + 1, W - 16),            # 4 W + 1 events: a last wavefront of 1
              (RUN + 1, RUN, W + 1, W - 1, W, 4, W - 14),         # 4 W + RUN - 1
              (W, W + 1, RUN, W - 1, RUN + 1, W - 8))             # 4 W + RUN + 1


@functools.lru_cache(maxsize=None)
def run_set(which):
    return G.scan_set(oracles.load_restatement(), RUN_COUNTS[which], seed=10 + which)


def check_runs(lib, O, which, tunes=TUNES):
    seqs, minsize, counts = run_set(which)
    ev = T.pair_events(O, seqs, minsize)
    assert tuple(len(e) for e in ev) == counts, [len(e) for e in ev]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert sum(counts) % W == (1, RUN - 1, RUN + 1)[which]
    if which == 0:
        assert {0, RUN - 1} <= {int(s) % RUN for s in starts}          # a pair opens on the first event of a run of RUN and on its last
    if which == 1:
        assert {1, 2, 5} <= {int(s) % RUN for s in starts}              # ... on its second and on middle ones
    if which == 2:
        assert W in starts                                              # ... and on a wavefront's first lane
    want, reported = T.check_candidates(lib, O, "runs%d" % which, seqs, minsize, tunes)
    assert reported == sum(counts) and len(want[0]) >= 3, (reported, len(want[0]))      # (the shortest genome holds 4 or 8 events: few multi-MUMs)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_runs_inside_a_lane(libs, which):
    check_runs(libs[0], libs[1], which)


# ------------------------------------------------------------------------------------------ carries
def planted_n(ref, count, lengths=(23, 25, 24)):
    """a query that is N but for `count` stretches of the reference (their lengths cycled), one N after each: exactly `count`
    events on diagonal 0 at a minimum length of 22, as long as chance adds none (4^-22 per pair of positions: the callers count)"""
    q = bytearray()
    for i in range(count):
        L = lengths[i % len(lengths)]
        q += ref[len(q):len(q) + L] + b"N"
    return bytes(q)


@functools.lru_cache(maxsize=None)
def carry_set(wave, seed=0):
    """(seqs, minsize, counts): with `wave` events per wavefront, a pair that ends with the first chunk of SummaryCarry, a pair over
    the next two chunks and one wavefront more (its carry into the last chunk joins two rounds of summaries), and a pair that ends
    with that chunk"""
    chunk = CARRY_TILES * wave
    counts = (chunk, 2 * chunk + wave, chunk - wave)
    rng = np.random.default_rng(9000 + seed)
    ref = random_seq(rng, 25 * max(counts) + 40)
    return [ref] + [planted_n(ref, c) for c in counts], 22, counts


def check_carries(lib, O, wave, tunes=TUNES, count_every_pair=True):
    """count_every_pair = False (the device's size, 32 768 events): the pairs' counts are not taken from the restatement one by
    one (seconds) -- the planted stretches are the design, and the engine's total equals their number only if chance added none"""
    seqs, minsize, counts = carry_set(wave)
    chunk = CARRY_TILES * wave
    ends = np.cumsum(counts)
    assert ends[0] == chunk and ends[2] == 4 * chunk and counts[1] > 2 * chunk
    if count_every_pair:
        ev = T.pair_events(O, seqs, minsize)
        assert tuple(len(e) for e in ev) == counts, [len(e) for e in ev]
    want, reported = T.check_candidates(lib, O, "carries", seqs, minsize, tunes)
    assert reported == sum(counts) and len(want[0]) >= min(counts) // 2, (reported, len(want[0]))      # (the shortest genome's stretches are in all three)
    # the long pair alone: its events as the engine lists them (pm_find_events runs the same order and scan)
    q = seqs[2]
    fwd = T.want_events(O, seqs[0], q, minsize)
    assert len(fwd) == counts[1] and T.got_events(lib, seqs[0], q, minsize, 0) == fwd
    if count_every_pair:
        assert T.got_events(lib, seqs[0], q, minsize, 1) == T.want_events(O, seqs[0], oracles.revcomp(q), minsize)


def test_carries_across_chunks(libs):
    check_carries(libs[0], libs[1], EMU_WAVE)


@functools.lru_cache(maxsize=None)
def no_carry_set(wave, seed=0):
    rng = np.random.default_rng(9100 + seed)
    counts = (wave,) * 6
    ref = random_seq(rng, 27 * wave + 40)
    return [ref] + [planted_n(ref, c, lengths=(23 + g % 3, 25, 24)) for g, c in enumerate(counts)], 22, counts


def check_no_carry(lib, O, wave, tunes=TUNES):
    """every wavefront's first event opens a pair: no carry is used anywhere"""
    seqs, minsize, counts = no_carry_set(wave)
    ev = T.pair_events(O, seqs, minsize)
    assert tuple(len(e) for e in ev) == counts, [len(e) for e in ev]
    want, reported = T.check_candidates(lib, O, "no_carry", seqs, minsize, tunes)
    assert reported == sum(counts) and len(want[0]) >= min(wave, 40) // 2, (reported, len(want[0]))      # (three phases of stretches: the six genomes share about a tenth of them)


def test_every_wavefront_opens_a_pair(libs):
    check_no_carry(libs[0], libs[1], EMU_WAVE)


def test_wavefronts_in_any_order(libs, monkeypatch):
    """the wavefronts of SummaryCarry and of WaveScan depend on pass 1 alone, not on one another: last to first, the same result"""
    for launch in ("summary_carry", "wave_scan", "coarse_from_buckets"):
        monkeypatch.setenv("PM_EMU_REVERSE_WAVES", launch)
        check_carries(libs[0], libs[1], EMU_WAVE, ({},))


# ------------------------------------------------------------------------------------------ the coarse table
REGION_LENGTHS = (255, 256, 257, 64 * 256 + 1)
NQS = (1, 63, 64, 65, 200)
COARSE_CASES = [(n, nq) for n in REGION_LENGTHS for nq in NQS if n < 1000 or nq in (1, 65, 200)]


@functools.lru_cache(maxsize=None)
def population(n, nq):
    rng = np.random.default_rng(100 * n + nq)
    ref = random_seq(rng, n)
    qs = [mutate(rng, ref, sub=0.03) for _ in range(nq)]
    for g in range(2, nq, 7):      # some genomes end early or begin late: pairs without events in the first or the last blocks
        qs[g] = qs[g][:n // 2] if g % 2 else qs[g][n // 2:]
    return [ref] + qs


def check_coarse(lib, O, n, nq, tunes=TUNES):
    seqs = population(n, nq)
    rows = (n + G.BLOCK - 1) // G.BLOCK + 1
    assert rows == {255: 2, 256: 2, 257: 3}.get(n, 66) and (rows <= COARSE_ROWS or rows % COARSE_ROWS == 2)      # (66 rows: a last tile of two, the last row of the region in it)
    want, reported = T.check_candidates(lib, O, "coarse", seqs, 11, tunes)
    assert reported > nq and (len(want[0]) > 0 or nq > 60), (reported, len(want[0]))


@pytest.mark.parametrize("n,nq", COARSE_CASES)
def test_coarse_table(libs, n, nq):
    check_coarse(libs[0], libs[1], n, nq)


def one_block_batch(seed, nq, n_regions, long_every=0):
    """(seqs, starts, lens, mins): regions of at most 256 reference positions -- one block, two rows of the table each; up to 128
    bases on every side (the grouped form takes them) or more (it does not); with long_every, a region of several blocks among them"""
    rng = np.random.default_rng(seed)
    glen = 9000
    ref = random_seq(rng, glen)
    qs = [mutate(rng, ref, sub=0.03) for _ in range(nq)]
    seqs = [ref] + qs
    starts = np.zeros((n_regions, nq + 1), np.int64); lens = np.zeros_like(starts); mins = np.zeros(n_regions, np.int32)
    for r in range(n_regions):
        if long_every and r % long_every == long_every - 1:
            ln = int(rng.integers(257, 2500))
        else:
            ln = int(rng.integers(1, 129)) if r % 2 else int(rng.integers(129, 257))
        st = int(rng.integers(0, glen - ln))
        for g in range(nq + 1):
            starts[r, g] = st; lens[r, g] = max(0, ln - (int(rng.integers(0, 4)) if g and rng.random() < 0.2 else 0))
        mins[r] = int(rng.integers(6, 12))
    return seqs, starts, lens, mins


def check_one_block_batch(lib, O, seed, nq, n_regions, long_every, every=5):
    seqs, starts, lens, mins = one_block_batch(seed, nq, n_regions, long_every)
    got = {}
    for grouped in (1, 0):
        for how in (1, 0):
            with Session(lib, seqs) as s:
                s.tune("group_small", grouped); s.tune("bucket_sort", how)
                got[grouped, how] = s.multi_mum_batch(starts, lens, mins)
                counts = dict(s.last_timing())
            assert (counts.get("n_grouped", 0) > 0) == bool(grouped), counts
    n = 0
    for r in range(n_regions):
        for key in got:
            assert T.same(got[1, 1][r], got[key][r]), (r, key, starts[r], lens[r], mins[r])
        if r % every == 0 or r == n_regions - 1:      # (the last region: the last rows of the table)
            sub = [seqs[g][starts[r, g]:starts[r, g] + lens[r, g]] for g in range(nq + 1)]
            want = oracles.restatement_multi_mum(O, sub, int(mins[r]), 1)
            assert T.same(want, got[1, 1][r]), (r, starts[r], lens[r], mins[r])
            n += len(want[0])
    return n


@pytest.mark.parametrize("nq,long_every,floor", [(5, 0, 20), (70, 0, 5), (9, 11, 20)])      # (70 genomes at 3 % divergence share few stretches)
def test_one_block_regions(libs, nq, long_every, floor):
    assert check_one_block_batch(libs[0], libs[1], 40 + nq, nq, 300 if nq < 20 else 120, long_every) > floor


# ------------------------------------------------------------------------------------------ the cursors
def cursor_sets():
    """{name: (seqs, minsize)}: empty buckets at the very beginning and the very end of the bucket range; a bucket of more than 64
    events (a run over wavefronts of EventPlace); events in the last bucket only"""
    rng = np.random.default_rng(77)
    n = 5 * G.BLOCK + 40
    ref = random_seq(rng, n)
    nothing = b"N" * 300
    mid = b"N" * 600 + ref[600:900] + b"N" * 300
    out = {"empty_ends": ([ref, mid, mutate(rng, ref, sub=0.02), mid], 10)}
    stretch = ref[G.BLOCK + 20:G.BLOCK + 32]
    out["long_bucket"] = ([ref, (stretch + b"N") * 150 + ref[700:1000], ref[:900], (stretch + b"N") * 70], 10)
    tail = ref[n - 30:]
    out["last_bucket"] = ([ref, nothing, nothing, b"N" * 50 + tail], 10)
    return out


def check_cursors(lib, O, name, tunes=TUNES):
    seqs, minsize = cursor_sets()[name]
    ev = T.pair_events(O, seqs, minsize)
    blocks = [sorted({e[0] >> 8 for e in x}) for x in ev]
    last = (len(seqs[0]) - 1) >> 8
    if name == "empty_ends":
        assert blocks[0] and blocks[0][0] > 0 and blocks[2] and blocks[2][-1] < last, blocks
    if name == "long_bucket":
        assert max(np.bincount([e[0] >> 8 for e in ev[0]])) > 128 and max(np.bincount([e[0] >> 8 for e in ev[2]])) > 64
    if name == "last_bucket":
        assert blocks == [[], [], [last]], blocks
    want, reported = T.check_candidates(lib, O, name, seqs, minsize, tunes)
    assert reported == sum(len(e) for e in ev)
    for q in seqs[1:]:
        if len(q) > G.SMALL:
            for strand in (0, 1):
                assert T.got_events(lib, seqs[0], q, minsize, strand) == T.want_events(O, seqs[0], oracles.revcomp(q) if strand else q, minsize), (name, strand)


@pytest.mark.parametrize("name", ["empty_ends", "long_bucket", "last_bucket"])
def test_cursors(libs, name):
    check_cursors(libs[0], libs[1], name)
