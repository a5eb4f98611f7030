"""The SUFFIX-ARRAY path of the event search at its round and segment edges, in the kernel emulation: DenseRank0, DenseKeys, DenseHeads,
DenseRerank, DenseLcp, DenseRep and SeedDense (parsnp_amd/csrc/engine/dense_kernels.h) with dense_build and the re-run logic of
Engine::run (engine_core.h), on the designed inputs of tests/densegen.py.  tests/test_gpu_dense_edges.py runs the same checks through
libparsnp_hip.so, where the radix sort is given a bit range (the emulation's sort_pairs ignores it) and the slices' atomics order
the events.  The path is selected with `dense_all`: PARSNP_TUNE for pm_find_events (which opens a session of its own), Session.tune
for sessions; that it ran is asserted on a Session of every case (`dense_regions`) and shown by the mutations of DESIGN.md 7.

(A) rep' at EVERY position: one query of probes per reference (densegen.probe_query) exposes rep'[l] as the ev_rep of the event
    (l, j, rep'[l] + 1); compared with the naive Python rep' and, as a whole event list, with the restatement.  References of 1, 2, 3,
    31 .. 33, 63 .. 65, 127 .. 129, 255 .. 257 bases, random, a tandem of period 8, a homopolymer run, X + G + X, N runs of 1, 2 and 33,
    one symbol throughout; L = 1 (every rep' visible) and L = 8, 16, 17 with planted repeats of K - 1, K, K + 1 bases.
(B) rounds: one planted repeat of 2^r - 1, 2^r, 2^r + 1 bases, r = 1 .. 9: `dense_rounds` is exactly the prediction from the naive
    longest repeat; as a batch with the longest first, in the middle and last, and a batch told apart after one round.
(C) SeedDense event by event (pm_find_events == restatement_events as sorted (l, j, len, rep'), both strands, the query as planted
    and reverse-complemented; a failure names case, L, strand and the first differing event): the catalogue of searchgen.py on this
    path; the binary search below / above every suffix, c == rlen, c == qlen, both, llo == lhi; left-maximality at j0 == 0, l0 == 0;
    ms == rep' and rep' + 1; the owner windows at strides 1, 2, 3, 16; the tail rule at minlen - 1, minlen, minlen + 1; N; a queue
    that overflows so that the pass repeats with SeedDense in it.
(D) batches of flagged regions against restatement_multi_mum per region, group_small 1 and 0, one genome stored reverse-complemented:
    equal regions adjacent and apart, three regions cut out of one tandem array, regions of 0 and 1 bases, every ref_pos & 31, a
    query piece cut at a match's first base, a region that ends with a copy of bases it holds before (the suffix that ends must sort
    before the one that goes on, whatever the next region begins with); 13 and 205 regions whose last holds an N (5 * nflag - 1 =
    64 and 1 024) with dense lengths 255 .. 257 and 1 023 .. 1 025 (the bit range of the device's sort); a batch that a work budget
    of 48 splits.
(E) six calls of one session: 9 rounds, 2 rounds, 9 again, 11 regions, 2 regions, 11 again; and a call over 200 bases after one over
    300, designed so that the first call's rank and LCP at element 200 -- which only a read past a segment meets -- would each cost
    a multi-MUM (the buffers have slack, so no sanitizer sees such a read).
tests/emu/dense_edges_check.cpp replays (A), (C) and (D) as a program of its own under AddressSanitizer and UBSan."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import densegen as G
import oracles
import test_search_edges as S
from parsnp_amd.binding import Lib, Session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


_want = {}


def want_events(O, ref, q, L):
    """the restatement's events of one strand: sorted (l, j, len, rep'), rep' zeroed below K; once per (ref, query, L) of a process"""
    key = (ref, q, L)
    if key not in _want:
        j, l, n, r = oracles.restatement_events(O, ref, q, L)
        _want[key] = sorted(zip(l.tolist(), j.tolist(), n.tolist(), [G.engine_rep(x, L) for x in r.tolist()]))
    return _want[key]


def got_events(lib, ref, q, L, strand):
    with G.dense_all():
        j, l, n, r = lib.find_events(ref, q, L, strand)
    return sorted(zip(l.tolist(), j.tolist(), n.tolist(), r.tolist()))


def session_counts(lib, seqs, L):
    """the counts of a Session opened under the same environment, on the anchor call"""
    with G.dense_all():
        with Session(lib, seqs) as s:
            s.whole(L)
            return dict(s.last_timing())


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4]))


# ------------------------------------------------------------------------------------------ (A) rep' at every position
@functools.lru_cache(maxsize=None)
def a_refs():
    return {a.name: a for a in G.a_references()}


@functools.lru_cache(maxsize=None)
def a_rep(name):
    return tuple(G.naive_rep(a_refs()[name].ref))


A_NAMES = tuple(a.name for a in G.a_references())


def check_rep(lib, O, name):
    a, rep = a_refs()[name], a_rep(name)
    for L in a.Ls:
        q, probes = G.probe_query(a.ref, rep, L)
        for strand in (0, 1):
            query = oracles.revcomp(q) if strand else q      # (strand 1 reads the probes from the mirrored piece)
            want = want_events(O, a.ref, q, L)
            got = got_events(lib, a.ref, query, L, strand)
            by = {(e[0], e[1]): e for e in got}
            for l, (j, b) in probes.items():
                assert by.get((l, j)) == (l, j, b, G.engine_rep(rep[l], L)), "%s, L %d, strand %d, position %d: rep' is %d by the naive suffix order, the probe's event is %s" % (
                    name, L, strand, l, rep[l], by.get((l, j)))
            assert got == want, "%s, L %d, strand %d: %s" % (name, L, strand, S.first_difference(want, got))
        t = session_counts(lib, [a.ref, q], L)
        assert t.get("dense_regions") == 1 and t.get("dense_rounds") == G.predicted_rounds([a.ref]), (name, L, t)


@pytest.mark.parametrize("name", A_NAMES)
def test_rep_at_every_position(libs, name):
    check_rep(libs[0], libs[1], name)


# ------------------------------------------------------------------------------------------ (B) rounds
@functools.lru_cache(maxsize=None)
def round_case(p):
    return G.round_case(p)


def check_rounds(lib, O, r):
    for p in ((1 << r) - 1, 1 << r, (1 << r) + 1):
        c = round_case(p)
        want = oracles.restatement_multi_mum(O, [c.ref, c.query], c.minsize, 1)
        with Session(lib, [c.ref, c.query]) as s:
            s.tune("dense_all", 1)
            got = s.whole(c.minsize)
            t = dict(s.last_timing())
        assert same(want, got), (c.name, first_candidate(want, got))
        assert t.get("dense_regions") == 1, (c.name, t)
        assert t.get("dense_rounds") == G.predicted_rounds([c.ref]), "%s: %d bases, longest repeat %d: %d rounds predicted, the engine took %s" % (
            c.name, len(c.ref), G.longest_repeat(c.ref), G.predicted_rounds([c.ref]), t.get("dense_rounds"))


def first_candidate(want, got):
    for i in range(min(len(want[0]), len(got[0]))):
        if any(not np.array_equal(want[x][i], got[x][i]) for x in range(4)):
            return "candidate %d (k, len, sp, fwd): restatement %s, engine %s" % (i, [want[x][i].tolist() for x in range(4)], [got[x][i].tolist() for x in range(4)])
    return "%d candidates, the restatement has %d" % (len(got[0]), len(want[0]))


@pytest.mark.parametrize("r", range(1, 10))
def test_rounds(libs, r):
    check_rounds(libs[0], libs[1], r)


# ------------------------------------------------------------------------------------------ (D) batches (used by (B) as well)
_mums = {}


def want_mums(O, b):
    """the restatement's multi-MUMs of every region; once per batch of a process, never changed"""
    if b.name not in _mums:
        _mums[b.name] = [oracles.restatement_multi_mum(O, G.pieces(b, r), int(b.mins[r]), 1) for r in range(b.starts.shape[0])]
    return _mums[b.name]


def run_batch(lib, b, tunes):
    with Session(lib, b.seqs) as s:
        for k, v in tunes.items():
            s.tune(k, v)
        got = s.multi_mum_batch(b.starts, b.lens, b.mins)
        return got, dict(s.last_timing())


def check_batch(lib, O, b, twice=False, tunes=None, rounds=True):
    """every region == the restatement with the small regions grouped and not; twice (the device): each a second time in a fresh
    session, identical bytes.  Returns the counts of the grouped run."""
    want = want_mums(O, b)
    nreg = b.starts.shape[0]
    out = None
    for grp in (1, 0):
        tn = dict(tunes or {"dense_all": 1}, group_small=grp)
        got, t = run_batch(lib, b, tn)
        for r in range(nreg):
            assert same(want[r], got[r]), "%s, region %d (%s), lengths %s, L %d, group_small %d: %s" % (
                b.name, r, b.info["rows"][r][0], b.lens[r].tolist(), b.mins[r], grp, first_candidate(want[r], got[r]))
        if "dense_all" in tn:
            assert t.get("dense_regions") == nreg, (b.name, grp, t)
            if rounds:
                assert t.get("dense_rounds") == G.predicted_rounds([G.pieces(b, r)[0] for r in range(nreg)]), (b.name, grp, t)
        if twice:
            again, _ = run_batch(lib, b, tn)
            for r in range(nreg):
                assert same(got[r], again[r]), (b.name, r, grp, "a second session gives other bytes")
        out = out or t
    assert sum(len(w[0]) for w in want) > 0, (b.name, "the batch holds no candidate")
    return out


@functools.lru_cache(maxsize=None)
def round_batches():
    return G.round_batches()


ROUND_BATCHES = ("longest_first", "longest_middle", "longest_last", "one_round")


def check_round_batch(lib, O, name, twice=False):
    b, at = round_batches()[name]
    each = [G.predicted_rounds([G.pieces(b, r)[0]]) for r in range(b.starts.shape[0])]
    if at is None:
        assert set(each) == {1}, each
    else:
        assert each[at] == 6 and max(each[:at] + each[at + 1:]) < 6 and b.info["rows"][at][0] == "long", (name, each)
    t = check_batch(lib, O, b, twice)
    assert t["dense_rounds"] == max(each), (name, t, each)


@pytest.mark.parametrize("name", ROUND_BATCHES)
def test_rounds_of_a_batch(libs, name):
    check_round_batch(libs[0], libs[1], name)


@functools.lru_cache(maxsize=None)
def segment_batch():
    return G.segment_batch()


def segment_floors(b):
    what = [row[0] for row in b.info["rows"]]
    nreg = len(what)
    assert {int(b.starts[r, 0]) & 31 for r in range(nreg) if what[r].startswith("align/")} == set(range(32))
    zero = [r for r in range(nreg) if b.lens[r, 0] == 0]
    assert zero[0] == 0 and zero[-1] == nreg - 1 and len(zero) == 3 and 0 < zero[1] < nreg - 1, zero
    assert sum(b.lens[r, 0] == 1 for r in range(nreg)) == 2
    same_ = [G.pieces(b, r)[0] for r in range(nreg) if what[r].startswith("same/")]
    assert len(same_) == 3 and len(set(same_)) == 1
    a0, a1 = what.index("same/adjacent0"), what.index("same/adjacent1")
    assert b.starts[a0, 0] + b.lens[a0, 0] == b.starts[a1, 0] and b.starts[what.index("same/apart"), 0] > b.starts[a1, 0] + b.lens[a1, 0]
    tn = [r for r in range(nreg) if what[r].startswith("tandem/")]      # cut out of ONE array: a suffix of one goes on into the next
    assert tn == [tn[0], tn[0] + 1, tn[0] + 2]
    arr = b.seqs[0][int(b.starts[tn[0], 0]):int(b.starts[tn[2], 0] + b.lens[tn[2], 0])]
    assert arr == arr[:8] * (len(arr) // 8) and all(b.lens[r, 0] > 128 for r in tn)
    e = what.index("left_edge")           # the piece begins 7 bases into the window, behind a base equal to the reference's
    for g in (1, 2):
        fwd = oracles.revcomp(b.seqs[g]) if g in b.info["reversed"] else b.seqs[g]
        st = b.info["rows"][e][2][g][0]
        assert st == b.starts[e, 0] + 7 and fwd[st - 1] == b.seqs[0][st - 1] and fwd[st:st + 40] == b.seqs[0][st:st + 40]
    assert 2 in b.info["reversed"]
    p = what.index("keys/prefix")         # the region ends with Y, holds Y + Z before, and is not the last region with bases
    s = G.pieces(b, p)[0]
    assert s[140:] == s[40:60] and G.naive_rep(s)[40] == 20 and len(s) > 128 and any(b.lens[r, 0] > 0 for r in range(p + 1, nreg))
    sa = G.suffix_order(s)
    assert sa.index(140) + 1 == sa.index(40)      # by the rule of DenseKeys the suffix that ends comes first, right before Y + Z
    for g in (1, 2):
        piece = G.pieces(b, p)[g]
        piece = oracles.revcomp(piece) if g in b.info["reversed"] else piece
        assert piece[60:85] == s[40:65] and piece[85:86] == b"T" > s[65:66]


def check_segments(lib, O, twice=False):
    b = segment_batch()
    segment_floors(b)
    want = want_mums(O, b)
    what = [row[0] for row in b.info["rows"]]
    e, p = what.index("left_edge"), what.index("keys/prefix")
    assert any(k == 7 and n > 100 for k, n in zip(want[e][0].tolist(), want[e][1].tolist())), (want[e][0], want[e][1])
    assert (40, 25) in zip(want[p][0].tolist(), want[p][1].tolist()), (want[p][0], want[p][1])
    check_batch(lib, O, b, twice)


def test_segments(libs):
    check_segments(*libs)


@functools.lru_cache(maxsize=None)
def width_batch(nflag, n):
    return G.width_batch(nflag, n)


def width_floors(b, nflag, n):
    assert b.starts.shape[0] == nflag and int(b.lens[:, 0].sum()) == n and 5 * nflag - 1 in (64, 1024)
    assert b"N" in G.pieces(b, nflag - 1)[0] and all(b"N" not in G.pieces(b, r)[0] for r in range(nflag - 1))
    assert n - 1 in (254, 255, 256, 1022, 1023, 1024)
    # every rank in use: 5 * nflag - 1 is the last region's N in round 0, n - 1 the largest suffix of the last round


def check_width(lib, O, nflag, n, twice=False):
    b = width_batch(nflag, n)
    width_floors(b, nflag, n)
    check_batch(lib, O, b, twice)


@pytest.mark.parametrize("nflag,n", G.WIDTHS)
def test_sort_width(libs, nflag, n):
    check_width(libs[0], libs[1], nflag, n)


@functools.lru_cache(maxsize=None)
def budget_batch():
    return G.budget_batch()


def check_budget(lib, O, twice=False):
    """measured in the kernel emulation: dense_regions = 3 (the three arrays), budget_retries = 1"""
    b = budget_batch()
    nreg = b.starts.shape[0]
    assert 38 <= nreg <= 42 and [r for r in range(nreg) if b.info["rows"][r][0] == "array"] == [0, nreg // 2, nreg - 1]
    t = check_batch(lib, O, b, twice, tunes={"work_budget": 48})
    print("budget batch:", {k: v for k, v in t.items() if k.startswith("dense") or k == "budget_retries"})
    assert t.get("budget_retries", 0) >= 1 and 2 <= t.get("dense_regions", 0) < nreg, t


def test_budget_splits_a_batch(libs):
    check_budget(*libs)


# ------------------------------------------------------------------------------------------ (C) SeedDense
@functools.lru_cache(maxsize=None)
def dense_pairs():
    return G.dense_pairs()


def designed_floors(O, p):
    """from the restatement alone: the designed events are events wherever the design says so, the suppressed ones are not, and
    every case holds an event; returns the number of (stretch, L) that had to be, and were, events"""
    floors = 0
    for L in p.Ls:
        fwd = want_events(O, p.ref, p.query, L)
        for l, j, n, kind in p.designed:
            at = [e for e in fwd if e[1] == j]
            if kind == "event" and n >= L:
                assert (l, j, n) in [e[:3] for e in at], (p.name, L, (l, j, n), "the designed stretch is not among the restatement's events", at)
                floors += 1
            else:
                assert not at, (p.name, L, (l, j, n), "must not be an event", at)
    assert any(want_events(O, p.ref, p.query, L) for L in p.Ls), (p.name, "holds no event")
    return floors


def check_pair(lib, O, p, half=None):
    floors = designed_floors(O, p)
    for L in p.Ls:
        for turned in (0, 1):
            query = oracles.revcomp(p.query) if turned else p.query
            for strand in (0, 1):
                if half is not None and strand != (turned + half + L) % 2:
                    continue
                want = want_events(O, p.ref, oracles.revcomp(query) if strand else query, L)
                got = got_events(lib, p.ref, query, L, strand)
                assert got == want, "%s, L %d, query %s, strand %d: %s" % (p.name, L, "reverse-complemented" if turned else "as planted", strand, S.first_difference(want, got))
    t = session_counts(lib, [p.ref, p.query], p.Ls[0])
    assert t.get("dense_regions") == 1 and t["rest_samples"] > 0, (p.name, t)      # (the samples are queued: SeedDense has items)
    return floors


def check_family(lib, O, family, thin=False):
    cases = [p for name, p in dense_pairs().items() if name.split("/")[0] == family]
    assert cases, family
    floors = sum(check_pair(lib, O, p, half=x if thin else None) for x, p in enumerate(cases))
    assert floors >= len(cases), (family, floors)


@pytest.mark.parametrize("family", G.PAIR_FAMILIES)
def test_seed_dense(libs, family):
    check_family(libs[0], libs[1], family)


def check_catalogue(lib, O, minsize, family):
    """the designed pairs of searchgen.py (test_search_edges.py) again, on this path"""
    with G.dense_all():
        S.FAMILIES[family](lib, O, minsize)


@pytest.mark.parametrize("minsize,family", S.STREAM_CASES)
def test_catalogue_on_this_path(libs, minsize, family):
    check_catalogue(libs[0], libs[1], minsize, family)


def check_overflow(lib, O):
    """nearly every K-mer of the reference is held twice, so nearly every sample is queued.  The four wavefronts of a workgroup share a
    sub-queue (`slice = (unit >> 2) & (kSlices - 1)`), so rest_samples > (sub-queues in use) x (a sub-queue's first capacity) means
    that one of them overflowed and the pass ran again, SeedDense included.  (All kSlices sub-queues together hold 131 072 samples,
    which queries of 2 000 bases cannot reach; the sub-queues in use are what counts.)"""
    ref, qs, L = G.overflow_pair()
    nunits = sum(G.units_of(len(q), L) for q in qs)
    cap = G.queue_first_capacity(nunits)
    in_use = -(-nunits // G.UNITS_PER_SLICE)
    want = oracles.restatement_multi_mum(O, [ref] + qs, L, 1)
    with Session(lib, [ref] + qs) as s:
        s.tune("dense_all", 1)
        got = s.whole(L)
        t = dict(s.last_timing())
    assert t["rest_samples"] > in_use * cap, (t["rest_samples"], in_use, cap)
    assert same(want, got) and len(want[0]) > 20, first_candidate(want, got)
    assert t.get("dense_regions") == 1, t


def test_queue_overflow(libs):
    check_overflow(*libs)


# ------------------------------------------------------------------------------------------ (E) calls in a row
def check_calls_in_a_row(lib, O):
    seqs, calls = G.calls_in_a_row()
    assert [c[0] for c in calls] == ["nine_rounds", "two_rounds", "nine_rounds", "eleven_regions", "two_regions", "eleven_regions"]
    first = {}
    with Session(lib, seqs) as s:
        s.tune("dense_all", 1)
        for step, (name, st, ln, mins) in enumerate(calls):
            got = s.multi_mum_batch(st, ln, mins)
            t = dict(s.last_timing())
            refs = [seqs[0][int(a):int(a + n)] for a, n in zip(st[:, 0], ln[:, 0])]
            rounds = G.predicted_rounds(refs)
            assert t.get("dense_regions") == len(refs) and t.get("dense_rounds") == rounds, (step, name, rounds, t)
            if name not in first:
                assert rounds == {"nine_rounds": 9, "two_rounds": 2}.get(name, rounds), (name, rounds)
                for r in range(len(refs)):
                    want = oracles.restatement_multi_mum(O, [x[int(a):int(a + n)] for x, a, n in zip(seqs, st[r], ln[r])], int(mins[r]), 1)
                    assert same(want, got[r]), (step, name, r, first_candidate(want, got[r]))
                first[name] = got
            else:
                assert all(same(a, b) for a, b in zip(first[name], got)), (step, name, "the second answer differs from the first")
    assert sum(len(x[0]) for g in first.values() for x in g) > 10


def test_calls_in_a_row(libs):
    check_calls_in_a_row(*libs)


def smaller_floors():
    """from the naive order alone: what the second call would read behind its arrays is what the first call left there, and it hurts"""
    seqs, calls, designed = G.smaller_after_larger()
    w1, w2 = seqs[0][:300], seqs[0][300:]
    rep = G.naive_rep(w2)
    assert rep[60] == 16 and rep[184] == 16 and w2[184:] == w2[60:76] and w1[200] == w2[76]      # Y, and c behind its first copy
    assert G.suffix_order(w2)[-1] == 120 and w2[120:121] == b"N" and rep[120] == 0                 # the largest suffix: the last SA position
    assert G.lcp_array(w1)[200] >= 30                                                              # the first call's lcp[200]
    assert G.predicted_rounds([w1]) > G.predicted_rounds([w2]) == 5                                # (every level the second call reads was written)
    return seqs, calls, designed


def check_smaller_after_larger(lib, O):
    seqs, calls, designed = smaller_floors()
    with Session(lib, seqs) as s:
        s.tune("dense_all", 1)
        for step, (st, ln, mins) in enumerate(calls):
            got = s.multi_mum_batch(st, ln, mins)[0]
            want = oracles.restatement_multi_mum(O, [x[int(a):int(a + n)] for x, a, n in zip(seqs, st[0], ln[0])], int(mins[0]), 1)
            if step == 1:
                assert set(designed) <= set(zip(want[0].tolist(), want[1].tolist())), (want[0], want[1])
            assert same(want, got), ("call %d" % step, first_candidate(want, got))


def test_smaller_call_after_a_larger(libs):
    check_smaller_after_larger(*libs)


# ------------------------------------------------------------------------------------------ floors and sources
def test_floors(cpu_checkers):
    """what the cases were designed to hold, from the naive Python rep' and the restatement alone (the engine is not loaded)"""
    O = oracles.load_restatement()
    # (B) every planted repeat length occurs as a reference's longest repeat
    assert {G.longest_repeat(round_case(p).ref) for p in G.ROUND_LENGTHS} == set(G.ROUND_LENGTHS)
    assert {G.predicted_rounds([round_case(p).ref]) for p in G.ROUND_LENGTHS} == set(range(1, 11))
    assert len(G.ROUND_LENGTHS) == 26 and G.ROUND_LENGTHS[-1] == 513      # (2^1 + 1 = 2^2 - 1)
    # (A) at most 5 % of a reference's positions go unprobed at L = 1; the planted repeats are what the naive rep' says; every probe is
    # one of the restatement's events and carries the naive rep'
    shown = {}
    for name in A_NAMES:
        a, rep = a_refs()[name], a_rep(name)
        q, probes = G.probe_query(a.ref, rep, 1)
        shown[name] = (len(probes), len(a.ref))
        if a.floor:
            assert len(a.ref) - len(probes) <= 0.05 * len(a.ref), (name, shown[name])
        else:
            assert sorted(probes) == [0] and len(set(a.ref)) == 1, name      # one symbol throughout: rep'[l] = n - l for l > 0
        assert all(rep[l] == p for l, p in a.planted), (name, a.planted)
        for L in a.Ls:
            q, probes = G.probe_query(a.ref, rep, L)
            fwd = set(want_events(O, a.ref, q, L))
            assert probes and all((l, j, b, G.engine_rep(rep[l], L)) in fwd for l, (j, b) in probes.items()), (name, L)
    print("positions probed at L = 1:", shown)
    for L in (8, 16, 17):
        K = G.params(L)[0]
        assert sorted({p for _, p in a_refs()["planted%d" % L].planted}) == [K - 1, K, K + 1]
    assert [len(a_refs()[n].ref) for n in A_NAMES[:15]] == [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    assert [a_refs()["nrun%d" % k].ref.count(b"N") for k in (1, 2, 33)] == [1, 2, 33]
    # (C) every case holds an event, the designed events are the restatement's; what the order cases are for, from the naive order
    for p in dense_pairs().values():
        assert not (len(p.ref) <= 128 and len(p.query) <= 128), p.name      # (a small pair never reaches SeedDense)
        designed_floors(O, p)
    ref_sym = lambda p: [G.symbols(p.ref)[i:] for i in range(len(p.ref))]
    p = dense_pairs()["order/below_all"]
    assert G.symbols(p.query[p.designed[0][1]:]) < min(ref_sym(p))
    p = dense_pairs()["order/above_all"]
    assert G.symbols(p.query[p.designed[0][1]:]) > max(ref_sym(p))
    p = dense_pairs()["order/tie"]
    l, j, n, _ = p.designed[0]
    sq = G.symbols(p.query[j:]); sa = sorted(ref_sym(p) + [sq]); at = sa.index(sq)
    assert [len(os.path.commonprefix([sq, x])) for x in (sa[at - 1], sa[at + 1])] == [n, n]      # llo == lhi
    for name in ("whole_suffix", "both_ends"):
        p = dense_pairs()["order/" + name]
        assert p.designed[0][0] + p.designed[0][2] == len(p.ref)
    for name in ("proper_prefix", "both_ends", "below_all"):
        p = dense_pairs()["order/" + name]
        assert p.designed[0][1] + p.designed[0][2] == len(p.query)
    for stride in (1, 2, 3, 16):
        p = dense_pairs()["owner/stride%d" % stride]
        assert G.params(p.Ls[0])[1] == stride and p.designed[0][1] == 0
        assert sorted({(-j) % stride for _, j, _, _ in p.designed[1:]}) == list(range(stride)) and len(p.designed) == stride + 2
    for L in (8, 17, 19):
        assert [len(dense_pairs()["tail/%d%+d" % (L, d)].query) - dense_pairs()["tail/%d%+d" % (L, d)].designed[0][1] for d in (-1, 0, 1)] == [L - 1, L, L + 1]
    # (D) every ref_pos & 31, the shapes, the sort widths
    segment_floors(segment_batch())
    for nflag, n in G.WIDTHS:
        width_floors(width_batch(nflag, n), nflag, n)
    assert {5 * f - 1 for f, _ in G.WIDTHS} == {64, 1024} and {n for _, n in G.WIDTHS} == {255, 256, 257, 1023, 1024, 1025}
    smaller_floors()
    # the queue overflow: more samples than the sub-queues in use hold at first
    ref, qs, L = G.overflow_pair()
    nunits = sum(G.units_of(len(q), L) for q in qs)
    assert [i for i in range(2000) if ref[i] != ref[2000 + i]] == list(range(25, 2000, 50)) and sum(len(q) for q in qs) > 2 * (-(-nunits // G.UNITS_PER_SLICE)) * G.queue_first_capacity(nunits)


def test_generator_matches_the_source():
    """the constants and rules densegen.py restates are those of the sources"""
    eng = os.path.join(ROOT, "parsnp_amd", "csrc", "engine")
    k = open(os.path.join(eng, "kernels.h")).read(); d = open(os.path.join(eng, "dense_kernels.h")).read(); e = open(os.path.join(eng, "engine_core.h")).read()
    assert int(re.search(r"constexpr int kDenseMaxLevels = (\d+);", d).group(1)) == G.DENSE_MAX_LEVELS
    assert int(re.search(r"constexpr int kSlices = (\d+);", k).group(1)) == G.SLICES
    per = int(re.search(r"#define PM_PER (\d+)", k).group(1))
    assert re.search(r"constexpr int kUnitSamples = 64 \* kPer;", k) and "constexpr int kPer = PM_PER;" in k and 64 * per == G.UNIT_SAMPLES
    assert int(re.search(r"#define PM_KMAX (\d+)", k).group(1)) == G.KMAX and "constexpr int kMaxK = PM_KMAX;" in k
    assert re.search(r"const int K = minlen < kMaxK \? minlen : kMaxK, stride = minlen - K \+ 1;", e)
    assert re.search(r"ri\.stride = ri\.minlen - ri\.K \+ 1;", e)
    assert [G.params(L) for L in (1, 8, 16, 17, 18, 31)] == [(1, 1), (8, 1), (16, 1), (16, 2), (16, 3), (16, 16)]
    assert re.search(r"c\.queue_cap = std::max<size_t>\(std::max<size_t>\(rest_cap_hint\[nreg == 1\], \(size_t\)nunits \* kUnitSamples / 16 / kSlices\), 64\) \+ 64;", e)
    assert G.queue_first_capacity(34) == 128 and G.queue_first_capacity(1 << 20) == (1 << 20) * 128 // 16 // 1024 + 64
    assert re.search(r"int64_t ns = \(ln\[g\] >= K && nR >= K && g >= g_first && g < g_last\) \? \(ln\[g\] - K\) / stride \+ 1 : 0;", e)
    assert re.search(r"units \+= \(ns \+ kUnitSamples - 1\) / kUnitSamples;", e)
    assert len(re.findall(r"const uint64_t slice = \(uint64_t\)\(\(unit >> 2\) & \(kSlices - 1\)\);", k)) == 1 and G.UNITS_PER_SLICE == 4
    assert "v >= ri.K ? v : 0" in d and "if (m - j0 < ri.minlen) continue;" in d
    assert "32 + bits_for(top_rank)" in e and "k == 0 ? (uint64_t)nflag * 5 : (uint64_t)n" in e


# ------------------------------------------------------------------------------------------ the sanitized program
def case_records(O):
    """(pair records, batches) for densegen.write_cases: (A) every reference at every L, (C) every designed pair at every L on both
    strands, (D) the segment batch, the sort-width batches and the batches of (B)"""
    pairs = []
    for name in A_NAMES:
        a, rep = a_refs()[name], a_rep(name)
        for L in a.Ls:
            q, _ = G.probe_query(a.ref, rep, L)
            pairs.append(("A/" + name, a.ref, q, L, 0, want_events(O, a.ref, q, L)))
    for p in dense_pairs().values():
        for L in p.Ls:
            for strand in (0, 1):
                pairs.append(("C/" + p.name, p.ref, p.query, L, strand, want_events(O, p.ref, oracles.revcomp(p.query) if strand else p.query, L)))
    batches = [segment_batch()] + [width_batch(f, n) for f, n in G.WIDTHS] + [round_batches()[n][0] for n in ROUND_BATCHES]
    return pairs, [(b, want_mums(O, b)) for b in batches]


def test_sanitized_program(cpu_checkers, tmp_path):
    """tests/emu/dense_edges_check.cpp: the cases of (A), (C) and (D) through pm_find_events and pm_multi_mum_batch of the emulation
    as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer, against the recorded restatement answers: a read
    that leaves a buffer ends it (one element past lcp[] or a rank array lies in the buffer's slack: test_smaller_call_after_a_larger)"""
    O = oracles.load_restatement()
    pairs, batches = case_records(O)
    cases = str(tmp_path / "cases.txt")
    G.write_cases(cases, O, pairs, batches)
    exe = str(tmp_path / "dense_edges_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPM_WAVE_EVENTS=5",
                    os.path.join(ROOT, "tests", "emu", "dense_edges_check.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k != "PARSNP_TUNE"}
    p = subprocess.run([exe, cases], capture_output=True, text=True, env=dict(env, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "dense_edges_check ok: %d pairs, %d batches" % (len(pairs), len(batches)) in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
