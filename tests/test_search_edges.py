"""The event search (parsnp_amd/csrc/engine/kernels.h: SeedExtend, SeedRest, the bucket order of the events, the wavefront scan) on
DESIGNED pairs (tests/searchgen.py) against the CPU restatement, event by event.  This module runs the cases in the kernel
emulation -- the sequential `#else` twins of the device bodies, and everything the two executions share (eq_up / eq_down, the
clamps, `reach`, the rep' test, win_join, EventOrder) -- and tests/test_gpu_search_edges.py runs the same bodies through
libparsnp_hip.so, where the `#if defined(__HIP_DEVICE_COMPILE__)` bodies execute.

What the lengths pin (K = min(minsize, 16), stride = minsize - K + 1, own = kPer * stride, unit = 64 * own):
  minsize - 1, minsize, + 1        below, at and above the reporting threshold (len >= minlen)
  64 - K - {1, 0, -1} (- stride)   a right arm that ends one base before, on and one base past the end of the lane's windows, for the
  64 - {1, 0, -1} (- stride)       lane's sample 0 and sample 1 (`reach`): as arm lengths and as whole stretches -- the cases
                                   `sample0` / `sample1` start every stretch on a lane's sample, so the stretch form ends on the edge
  31 .. 33, 63 .. 65, 95 .. 97     the three 32-base difference words; eq_up / eq_down handing over between them
  own - 1, own, own + 1            the first difference inside the lane's own bases or in its successor's (`first_diff < own`)
  unit - 1, unit, unit + 1,        starting on a wavefront's first lane: the run of lanes ends with lane 63 (`run_end`), the arm
  128 * stride + 40, + 70          ends inside lane 63's windows or past them (kOpenEnd, `cont`, the whole-wavefront loop)
  700 + L + 300, L = 2 047 .. 4 500   arms finished from memory: `n += 64 * 32; if (n >= cap) break`; `chunks`: the difference in
                                   lane chunk 0, 1 and 63 of a round and in round 1 (`f * 32 + c`)
Every case asserts FLOORS from the restatement's output -- the designed lengths are among the event lengths, the clamped match
ends with the sequence, the block populations and pair counts are the intended ones -- so a generator that stops reaching a path
turns the test red.  No case is a small_pair (both sides <= 128 bases go to SmallPairEvents and never reach SeedExtend).  At the
minimum lengths whose lanes hold windows (8 .. 31) every query piece is at least one unit long (m >= 128 * stride: `follow`),
except in the clamp case `m1x+-1`, one base short of it on purpose; at 32, 48 and 90 there is no `follow` at any length."""
import functools
import os
import re

import numpy as np
import pytest

import oracles
import searchgen as G
from parsnp_amd.binding import Lib, Session
from seqgen import adversarial_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


# ------------------------------------------------------------------------------------------ streams
_want = {}


def want_events(O, ref, q, min_len):
    """the restatement's events of one strand, as test_events compares them: sorted (l, j, len, rep'), rep' zeroed below K (the
    engine measures rep' along K-mer chains).  Computed once per (ref, query, min_len) of a process."""
    key = (ref, q, min_len)
    if key not in _want:
        K = min(min_len, G.KMAX)
        j, l, n, r = oracles.restatement_events(O, ref, q, min_len)
        _want[key] = sorted(zip(l.tolist(), j.tolist(), n.tolist(), [x if x >= K else 0 for x in r.tolist()]))
    return _want[key]


def got_events(lib, ref, q, min_len, strand):
    j, l, n, r = lib.find_events(ref, q, min_len, strand)
    return sorted(zip(l.tolist(), j.tolist(), n.tolist(), r.tolist()))


def first_difference(want, got):
    for i, (a, b) in enumerate(zip(want, got)):
        if a != b:
            return "event %d (l, j, len, rep'): restatement %s, engine %s" % (i, a, b)
    if len(want) > len(got):
        return "the engine misses event %d of %d: %s" % (len(got), len(want), want[len(got)])
    return "the engine adds event %d: %s" % (len(want), got[len(want)])


def check_streams(lib, O, name, ref, q, minsize):
    """pm_find_events == the restatement, both strands, the query as it is and reverse-complemented (the same matches through the
    reverse-strand path: kRev -> SeedRest)"""
    assert not (len(ref) <= G.SMALL and len(q) <= G.SMALL), (name, "a small_pair never reaches SeedExtend")
    for turned in (0, 1):
        query = oracles.revcomp(q) if turned else q
        for strand in (0, 1):
            want = want_events(O, ref, oracles.revcomp(query) if strand else query, minsize)
            got = got_events(lib, ref, query, minsize, strand)
            assert got == want, "%s, minsize %d, query %s, strand %d: %s" % (name, minsize, "reverse-complemented" if turned else "as planted", strand, first_difference(want, got))


def lens_of(events):
    return {e[2] for e in events}


@functools.lru_cache(maxsize=None)
def edge_pairs(minsize):
    return G.edge_pairs(minsize)


@functools.lru_cache(maxsize=None)
def long_arm_pairs(minsize):
    return G.long_arm_pairs(minsize)


def check_edges(lib, O, minsize):
    K, stride, own, unit = G.params(minsize)
    small, big = G.edge_lengths(minsize)
    for name, p in edge_pairs(minsize).items():
        fwd = want_events(O, p.ref, p.query, minsize)
        assert len(p.query) >= unit or not G.windows(minsize), (name, minsize)      # m >= 128 * stride: `follow` where the lanes hold windows
        designed = [r for r in p.recs if r[4]]
        assert {r[4] for r in designed} == set(small + big), (name, minsize)      # every length was planted ...
        starts = {(e[0], e[1]): e[2] for e in fwd}
        for a, b, n, kind, L in designed:                               # ... and is an event of its true length (a deletion may merge it with a base of its neighbour)
            if n >= minsize:
                assert starts.get((a, b)) == n, (name, minsize, "planted stretch of", L, "at", (a, b), "true length", n, "is not an event")
        if name != "mix":
            assert {x for x in small + big if x >= minsize} <= lens_of(fwd), (name, minsize)
            assert not any(r[2] != r[4] for r in designed), (name, minsize)
        else:
            assert {"sub", "ins", "del", "n"} <= {r[3] for r in designed}
        assert not any(n < minsize and (a, b) in starts for a, b, n, kind, L in designed)      # below the threshold: no event
        if name in ("sample0", "sample1"):
            phase = 0 if name == "sample0" else stride % own
            assert all(b % own == phase for a, b, n, kind, L in designed if L not in big), (name, minsize)
        if G.windows(minsize):
            assert all(b % unit == (stride % own if name == "sample1" else 0) for a, b, n, kind, L in designed if L in big), (name, minsize)
        check_streams(lib, O, "edges/" + name, p.ref, p.query, minsize)


def check_long_arms(lib, O, minsize):
    K, stride, own, unit = G.params(minsize)
    seen = set()
    for name, p in long_arm_pairs(minsize).items():
        fwd = want_events(O, p.ref, p.query, minsize)
        assert len(p.ref) < 20000 and (len(p.query) >= unit or not G.windows(minsize)), (name, minsize, len(p.ref))
        starts = {(e[0], e[1]): e[2] for e in fwd}
        for a, b, n, kind, L in p.recs:
            if L in G.LONG_ARMS or (L and name.startswith("chunks")):
                assert starts.get((a, b)) == n == L, (name, minsize, L, n)
                seen.add(L)
                if name.startswith("chunks"):
                    assert b % unit == 0, (name, minsize, L, b)      # from a wavefront's first lane, ending where designed
        check_streams(lib, O, "long/" + name, p.ref, p.query, minsize)
    assert set(G.LONG_ARMS) <= seen, (minsize, seen)
    if G.windows(minsize):
        assert {63 * own + 64 + t for t in (0, 31, 32, 2047, 2048)} <= seen, (minsize, seen)


def check_clamps(lib, O, minsize):
    K, stride, own, unit = G.params(minsize)
    for name, (ref, q) in G.clamp_pairs(minsize).items():
        fwd = want_events(O, ref, q, minsize)
        nR, m = len(ref), len(q)
        ends_q = any(e[1] + e[2] == m for e in fwd); ends_r = any(e[0] + e[2] == nR for e in fwd)
        if name == "query_is_prefix":
            assert any(e[1] + e[2] == m and e[2] >= 300 for e in fwd) and nR > m, (name, minsize)
        elif name == "reference_is_prefix":
            assert any(e[0] + e[2] == nR and e[2] >= 300 for e in fwd) and m > nR, (name, minsize)
        elif name == "identical":
            assert fwd == [(0, 0, nR, fwd[0][3])] and m == nR >= 2 * unit, (name, minsize)
        elif name.startswith("front"):
            assert any(e[0] == 0 and e[1] == int(name[5:]) for e in fwd), (name, minsize)       # starts on the reference's first base
        elif name.startswith("rfront"):
            assert any(e[1] == 0 and e[0] == int(name[6:]) for e in fwd), (name, minsize)       # ... on the query's
        else:
            k, r = name[1:].split("x+")
            assert m == unit * int(k) + int(r) and ends_q, (name, minsize, m)                   # the last match is cut by the end of the piece
        check_streams(lib, O, "clamps/" + name, ref, q, minsize)
        if name == "identical" and G.windows(minsize) and K == G.KMAX:
            # every sample is confirmed where its leader's probe predicts it -- the leaders at lane 0 and lane 64 - kLead of every
            # wavefront included -- so nothing is handed to SeedRest (16-mers of 4 kb of random sequence: none repeated, none its
            # own reverse complement), and the one arm that outruns its wavefront is finished by the whole-wavefront loop
            with Session(lib, [ref, q]) as s:
                s.whole(minsize)
                t = dict(s.last_timing())
            assert t["rest_samples"] == 0 and t["events"] == 1, (minsize, t)


def check_leaders(lib, O, minsize):
    K, stride, own, unit = G.params(minsize)
    quiet = 2 * G.KLEAD * own
    for name, (ref, q, spots) in G.leader_pairs(minsize).items():
        fwd = want_events(O, ref, q, minsize)
        assert len(q) >= unit
        for s in spots:
            first = s - K // 2                                          # the leader's first sample: the difference lies inside its K-mer
            lane = (first % unit) // own
            assert first % own == 0 and lane % G.KLEAD == 0 and lane in (0, 32, 64 - G.KLEAD), (name, minsize, s)
            # nothing else differs for 2 * kLead lanes on either side: one match ends on the planted difference, one begins after it
            assert any(e[0] + e[2] == s and e[2] >= quiet for e in fwd), (name, minsize, s)
            assert any(e[0] == s + (0 if name.endswith("ins") else 1) and e[2] >= quiet for e in fwd), (name, minsize, s)
        check_streams(lib, O, "leaders/" + name, ref, q, minsize)


def check_repeats(lib, O, minsize):
    K, stride, own, unit = G.params(minsize)
    ref, q, info = G.repeat_pair(minsize)
    fwd = want_events(O, ref, q, minsize)
    R, a = info["R"], info["a"]
    by_j = {e[1]: e for e in fwd}
    assert info["j_alone"] not in by_j, (minsize, "the copy alone (len == rep') must be suppressed")
    assert by_j.get(info["j_plus1"], (0, 0, 0, 0))[2:] == (R + 1, R), (minsize, by_j.get(info["j_plus1"]))      # len == rep' + 1
    assert any(e[0] <= a and e[0] + e[2] >= a + R and e[2] > 300 for e in fwd), minsize                     # the copy inside a long match
    pal = ref[info["pal_at"]:info["pal_at"] + K]
    assert pal == oracles.revcomp(pal) and info["pal_at"] % stride == 0 and q[info["pal_at"]:info["pal_at"] + K] == pal
    assert len(q) >= unit
    check_streams(lib, O, "repeats", ref, q, minsize)


FAMILIES = {"edges": check_edges, "long": check_long_arms, "clamps": check_clamps, "leaders": check_leaders, "repeats": check_repeats}
STREAM_CASES = [(m, f) for m in G.MINSIZES for f in FAMILIES if f != "leaders" or G.windows(m)]


@pytest.mark.parametrize("minsize,family", STREAM_CASES)
def test_event_streams(libs, minsize, family):
    FAMILIES[family](libs[0], libs[1], minsize)


def test_generator_matches_the_header():
    """the defaults searchgen.py restates are those of kernels.h: a changed default turns this red instead of moving the edges away
    from the planted lengths"""
    src = open(os.path.join(ROOT, "parsnp_amd", "csrc", "engine", "kernels.h")).read()
    for name, value in (("PM_PER", G.KPER), ("PM_LEAD", G.KLEAD), ("PM_KMAX", G.KMAX), ("PM_WAVE_EVENTS", G.WAVE_EVENTS)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == value, name
    assert int(re.search(r"kCoarseShift = (\d+)", src).group(1)) == 8 and G.BLOCK == 256
    assert re.search(r"small_pair\(int64_t nR, int64_t m\) \{ return nR <= 128 && m <= 128; \}", src) and G.SMALL == 128
    assert [G.params(m)[1] for m in G.MINSIZES] == [1, 1, 2, 4, 10, 16, 17, 33, 75]
    assert [G.windows(m) for m in G.MINSIZES] == [True] * 6 + [False] * 3


def check_adversarial_events(lib, O, count, seed):
    """test_events' inputs (planted repeats, N runs, two-letter alphabets, rotations, reverse-complemented segments) at 130 .. 700
    bases: no pair is a small_pair, so the events come from SeedExtend / SeedRest and the index walks"""
    rng = np.random.default_rng(seed)
    total = 0
    for it in range(count):
        ref, (q,) = adversarial_case(rng, 130, 700)
        min_len = int(rng.integers(1, 20))
        assert len(ref) > G.SMALL
        for strand in (0, 1):
            want = want_events(O, ref, oracles.revcomp(q) if strand else q, min_len)
            got = got_events(lib, ref, q, min_len, strand)
            assert got == want, "case %d, min_len %d, strand %d: %s\n%r\n%r" % (it, min_len, strand, first_difference(want, got), ref, q)
            total += len(want)
    assert total > 20 * count


def test_events_beyond_small_pairs(libs):
    check_adversarial_events(libs[0], libs[1], 120, 7)


# ------------------------------------------------------------------------------------------ candidate lists
def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def pair_events(O, seqs, minsize):
    """per query genome: the restatement's events of both strands"""
    return [want_events(O, seqs[0], q, minsize) + want_events(O, seqs[0], oracles.revcomp(q), minsize) for q in seqs[1:]]


def check_candidates(lib, O, name, seqs, minsize, tunes):
    """Session.whole == restatement_multi_mum under every setting of `tunes`; returns the event count the engine reports"""
    want = oracles.restatement_multi_mum(O, seqs, minsize, 1)
    reported = None
    for tune in tunes:
        with Session(lib, seqs) as s:
            for k, v in tune.items():
                s.tune(k, v)
            got = s.whole(minsize)
            reported = int(dict(s.last_timing())["events"])
        assert same(want, got), (name, minsize, tune, len(want[0]), len(got[0]))
    return want, reported


EMU_TUNES = ({}, {"bucket_sort": 0}, {"master_seg": 0})


def check_buckets(lib, O, tunes=EMU_TUNES):
    seqs, minsize, plan, edges = G.bucket_set()
    ev = pair_events(O, seqs, minsize)
    nblocks = (len(seqs[0]) + G.BLOCK - 1) // G.BLOCK
    for g, events in enumerate(ev):
        pop = np.bincount([e[0] >> 8 for e in events], minlength=nblocks)
        # the planted populations (an 8-mer that is repeated in the reference is no event; chance matches add some): every branch of
        # EventOrder -- 0, 1, 2, the register network at 3 .. 8 events, Shell's gaps above
        assert set(range(0, 10)) <= set(pop.tolist()) and (pop > 9).sum() >= 3 and pop.max() >= 25, (g, pop.tolist())
        assert {255, 0, 1} <= {e[0] % G.BLOCK for e in events}, g
    assert len(set(len(e) for e in ev)) > 1
    want, reported = check_candidates(lib, O, "buckets", seqs, minsize, tunes)
    assert reported == sum(len(e) for e in ev) and len(want[0]) > 100, (reported, len(want[0]))
    check_streams(lib, O, "buckets", seqs[0], seqs[1], minsize)


@functools.lru_cache(maxsize=None)
def scan_set(which):
    return G.scan_set(oracles.load_restatement(), G.SCAN_COUNTS[which])


def check_scan(lib, O, which, tunes=EMU_TUNES):
    seqs, minsize, counts = scan_set(which)
    ev = pair_events(O, seqs, minsize)
    assert tuple(len(e) for e in ev) == counts, [len(e) for e in ev]
    ends = np.cumsum(counts)
    assert (ends % G.WAVE_EVENTS == 0).sum() >= 2 and max(counts) > 3 * G.WAVE_EVENTS      # pairs that end on a wavefront's last lane; one that spans four
    assert all(any(e[0] != 0 for e in x) for x in ev)
    want, reported = check_candidates(lib, O, "scan%d" % which, seqs, minsize, tunes)
    assert reported == sum(counts) and len(want[0]) > 100, (reported, len(want[0]))


def check_ties(lib, O, tunes=EMU_TUNES):
    seqs, minsize = G.tie_set()
    for q in seqs[1:3]:
        fwd = want_events(O, seqs[0], q, minsize)
        reach = [(e[0], e[2]) for e in fwd]
        assert len(reach) > len(set(reach)), "two events of one pair and strand with the same l and the same reach"
    want, _ = check_candidates(lib, O, "ties", seqs, minsize, tunes)
    assert len(want[0]) >= 5
    for q in seqs[1:]:
        check_streams(lib, O, "ties", seqs[0], q, minsize)


def test_bucket_populations(libs):
    check_buckets(*libs)


@pytest.mark.parametrize("which", [0, 1])
def test_scan_carry(libs, which):
    """pairs of exactly 511, 512, 513, 1 024 and 1 537 events.  (The emulation's wavefronts hold 5 events, the device's 512: the
    counts are designed for the device, the emulation checks the inputs and the floors.)"""
    check_scan(libs[0], libs[1], which)


def test_equal_reach(libs):
    check_ties(*libs)
