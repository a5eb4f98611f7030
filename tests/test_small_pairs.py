"""The SMALL-REGION event search at its word and diagonal edges, in the kernel emulation: SmallPairEvents (kernels.h),
GroupedPairEvents and GroupedPairEventsWide (store_kernels.h) and what they share -- planes64, W64, W128, pair_diagonals -- on the
designed inputs of tests/smallgen.py against the CPU restatement.  tests/test_gpu_small_pairs.py runs the same checks through
libparsnp_hip.so, where the device bodies execute (LDS between the wave_syncs of the grouped forms, wave_reserve01, the slices'
atomics).

(a) one pair: pm_find_events == oracles.restatement_events as sorted (l, j, len, rep'), rep' zeroed below K = min(L, 16) as
    test_events does, both strands, the query as planted and reverse-complemented.  Every pair of 1, 2, 31 .. 33, 63 .. 65, 96, 127,
    128 bases and 128 x 129, 129 x 128, 129 x 129 (the first pairs that are NOT small: the three spellings of small_pair must
    agree on them); stretches of 1, 2, 31 .. 33, 63 .. 65, 127 bases, the shorter side's whole length and that minus 1, in the four
    corners and across bit 63 / 64; L = len - 1, len, len + 1 and two rotating values of 1 .. 5, 7 .. 9, 15 .. 17, 31 .. 33, 63 .. 65,
    127, 128 (the doubling filter of pair_diagonals at every k, with and without the rest step).
(b) batches: pm_multi_mum_batch with group_small = 0, group_small = 1 and group_wide = 1 on top, every region against
    restatement_multi_mum, the three routes byte for byte the same.  Which form takes which region is PREDICTED from the sources'
    limits and the restatement's events (predict()), and the counts of pm_last_timing must be the predicted ones: a generator that
    stops reaching a form, or a form that stops taking what it should, turns the test red.
A failure names the case, the lengths, the planted stretch, L, the strand or route and the first differing event or candidate."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracles
import smallgen as G
from parsnp_amd.binding import Lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs(emu, cpu_checkers):
    return Lib(emu[0]), oracles.load_restatement()


# ------------------------------------------------------------------------------------------ (a) one pair
_want = {}


def want_events(O, ref, q, L):
    """the restatement's events of one strand: sorted (l, j, len, rep'), rep' zeroed below K; once per (ref, query, L) of a process"""
    key = (ref, q, L)
    if key not in _want:
        K = min(L, G.KMAX)
        j, l, n, r = oracles.restatement_events(O, ref, q, L)
        _want[key] = sorted(zip(l.tolist(), j.tolist(), n.tolist(), [x if x >= K else 0 for x in r.tolist()]))
    return _want[key]


def first_difference(want, got):
    for i, (a, b) in enumerate(zip(want, got)):
        if a != b:
            return "event %d (l, j, len, rep'): restatement %s, engine %s" % (i, a, b)
    if len(want) > len(got):
        return "the engine misses event %d of %d: %s" % (len(got), len(want), want[len(got)])
    return "the engine adds event %d: %s" % (len(want), got[len(want)])


def covers(events, l, j, n):
    return any(e[0] - e[1] == l - j and e[0] <= l and e[0] + e[2] >= l + n for e in events)


def check_pair(lib, O, p, half=None):
    """both strands, the query as planted and reverse-complemented, at every L of the case; returns the number of (stretch, L) at
    which the designed stretch had to be, and was, among the restatement's events.  half (the device's thinned corner stretches, a
    session per call): two of the four calls -- the query as planted on one strand and reverse-complemented on the other, so that
    the planted bases are read from the forward and from the reverse strand's blocks; which way round alternates with half + L"""
    floors = 0
    nR, m = len(p.ref), len(p.query)
    for L in p.Ls:
        fwd = want_events(O, p.ref, p.query, L)
        for l, j, n in p.planted:
            if n >= L and G.occurrences(p.ref, p.ref[l:l + n]) == 1 and b"N" not in p.ref[l:l + n]:
                assert covers(fwd, l, j, n), (p.name, (nR, m), (l, j, n), L, "the designed stretch is not among the restatement's events", fwd)
                floors += 1
        for turned in (0, 1):
            query = oracles.revcomp(p.query) if turned else p.query
            for strand in (0, 1):
                if half is not None and strand != (turned + half + L) % 2:
                    continue
                want = want_events(O, p.ref, oracles.revcomp(query) if strand else query, L)
                jj, ll, nn, rr = lib.find_events(p.ref, query, L, strand)
                got = sorted(zip(ll.tolist(), jj.tolist(), nn.tolist(), rr.tolist()))
                assert got == want, "%s, lengths %d x %d, planted (l, j, n) %s, L %d, query %s, strand %d: %s" % (
                    p.name, nR, m, p.planted, L, "reverse-complemented" if turned else "as planted", strand, first_difference(want, got))
    return floors


def partners(nR):
    return [m for m in G.LENGTHS + (129,) if (nR, m) in G.OVER or (nR <= G.SMALL and m <= G.SMALL)]


def check_corners(lib, O, nR, thin):
    floors = calls = 0
    for m in partners(nR):
        cases = G.pair_cases(nR, m, thin)
        assert cases, (nR, m)
        for x, p in enumerate(cases):
            floors += check_pair(lib, O, p, half=x if thin else None)
            calls += (2 if thin else 4) * len(p.Ls)
    print("corner stretches, reference of %d bases: %d calls of pm_find_events, the designed stretch an event in %d (case, L)" % (nR, calls, floors))
    assert floors >= (1 if thin or nR < 8 else 30), (nR, floors)


@pytest.mark.parametrize("nR", G.LENGTHS + (129,))
def test_corner_stretches(libs, nR):
    check_corners(libs[0], libs[1], nR, thin=False)


def check_special(lib, O, family):
    S = {k: v for k, v in special().items() if k.split("/")[0].rstrip("0123456789x") == family}
    assert S, family
    for name, p in S.items():
        nR, m = len(p.ref), len(p.query)
        floors = check_pair(lib, O, p)
        ev = lambda L: want_events(O, p.ref, p.query, L)
        if family == "split":        # two events on one diagonal, one base apart
            (l1, j1, n1), (l2, j2, n2) = p.planted
            assert l1 + n1 + 1 == l2 and j1 + n1 + 1 == j2 and (j1 + n1 if l1 >= j1 else l1 + n1) in (63, 64), name
            at = {(e[0], e[1]): e[2] for e in ev(1)}
            assert at.get((l1, j1)) == n1 and at.get((l2, j2)) == n2, (name, at)
            assert floors == sum(n >= L for _, _, n in p.planted for L in p.Ls)
        elif family == "outer":      # d = -(m - L) and d = nR - L, at L - 1, L and L + 1 (where they are too short)
            L = p.planted[0][2]
            at = {(e[0], e[1]): e[2] for e in ev(L)}
            assert at.get((0, m - L)) == L and at.get((nR - L, 0)) == L, (name, at)
            assert not any(e[0] - e[1] in (L - m, nR - L) for e in ev(L + 1)), name
        elif family == "shorter":
            assert all(L > min(nR, m) and ev(L) == [] for L in p.Ls), name
        elif family == "whole":      # m == L or nR == L: one diagonal range of a single diagonal on that side
            assert p.Ls == (min(nR, m),) and floors == 1, (name, floors)
        elif name in ("n/reference", "n/query"):      # an N on one side ends the match: two events, none across it
            at = {(e[0], e[1]): e[2] for e in ev(4)}
            assert at.get((40, 44)) == 30 and at.get((71, 75)) == 29, (name, at)
        elif name == "n/both":       # N matches N: one event across it
            assert {(e[0], e[1]): e[2] for e in ev(4)}.get((40, 44)) == 60, name
        elif name == "n/run_to_end":
            assert covers(ev(1), 98, 70, 30), (name, ev(1))
        elif name == "repeat":
            by_j = {e[1]: e for e in ev(10)}
            assert 10 not in by_j, (name, "the copy alone (len == rep') must be suppressed", by_j.get(10))
            assert by_j.get(50) == (5, 50, 21, 20), (name, by_j.get(50))      # len == rep' + 1
        elif name == "homopolymer":
            assert all(ev(L) == [(0, 0, 128, 127)] for L in p.Ls), name
        elif name == "homopolymer/c":
            assert ev(16) == [], (name, ev(16))      # 127 x A lies twice in the reference: len == rep' at both places
        elif name == "homopolymer/c_ref":
            assert ev(16) == [(0, 0, 127, 126), (0, 1, 127, 126)], (name, ev(16))      # two query positions, one reference position, equal reach
        elif name == "tandem":
            assert len(ev(2)) >= 8, (name, len(ev(2)))      # (a lane's first event goes through wave_reserve01, its others through the slice's atomic)


@functools.lru_cache(maxsize=None)
def special():
    return G.special_pairs()


FAMILIES = ("split", "outer", "shorter", "whole", "n", "repeat", "homopolymer", "tandem")


@pytest.mark.parametrize("family", FAMILIES)
def test_special_pairs(libs, family):
    check_special(libs[0], libs[1], family)


# ------------------------------------------------------------------------------------------ (b) batches
@functools.lru_cache(maxsize=None)
def batch(name):
    return {"ends": G.ends_batch, "fields": G.fields_batch, "lanes70": lambda: G.lanes_batch(70), "lanes130": lambda: G.lanes_batch(130),
            "tandem": G.tandem_batch}[name]()


_mums = {}


def want_mums(O, b):
    """the restatement's multi-MUMs of every region; once per batch of a process, never changed"""
    if b.name not in _mums:
        _mums[b.name] = [oracles.restatement_multi_mum(O, G.pieces(b, r), int(b.mins[r]), 1) for r in range(b.starts.shape[0])]
    return _mums[b.name]


_pred = {}


def predict(O, b):
    """from the restatement's events and the limits the sources state: per region (form, events of all its pairs), form = "first"
    (all sides <= 128, at most kGrpPieces distinct pieces, at most kGrpEvents events of a (piece, strand)), "wide" (kWidePieces,
    kWideEvents) or "pairwise" (SmallPairEvents or the index)"""
    if b.name not in _pred:
        out = []
        for r in range(b.starts.shape[0]):
            sub = G.pieces(b, r); L = max(int(b.mins[r]), 1)
            if max(len(s) for s in sub) > G.SMALL:
                out.append(("pairwise", 0)); continue
            count = {}
            for q in set(sub[1:]):
                count[q] = [len(oracles.restatement_events(O, sub[0], x, L)[0]) if len(x) >= L and len(sub[0]) >= L else 0 for x in (q, oracles.revcomp(q))]
            worst = max(max(c) for c in count.values()); total = sum(sum(count[q]) for q in sub[1:])
            form = "first" if len(count) <= G.GRP_PIECES and worst <= G.GRP_EVENTS else "wide" if len(count) <= G.WIDE_PIECES and worst <= G.WIDE_EVENTS else "pairwise"
            out.append((form, total))
        _pred[b.name] = out
    return _pred[b.name]


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4]))


def first_candidate(want, got):
    for i in range(min(len(want[0]), len(got[0]))):
        if any(not np.array_equal(want[x][i], got[x][i]) for x in range(4)):
            return "candidate %d (k, len, sp, fwd): restatement %s, engine %s" % (i, [want[x][i].tolist() for x in range(4)], [got[x][i].tolist() for x in range(4)])
    return "%d candidates, the restatement has %d" % (len(got[0]), len(want[0]))


def check_batch(lib, O, b, twice=False):
    """every region on every route == the restatement (so the routes agree byte for byte), the counts of pm_last_timing are the
    predicted ones; twice (the device): every route a second time in a fresh session, identical bytes.  Returns the first run."""
    want = want_mums(O, b)
    pred = predict(O, b)
    runs = G.run_routes(lib, b)
    for route, (got, counts) in runs.items():
        for r in range(b.starts.shape[0]):
            assert same(want[r], got[r]), "%s, region %d (%s), lengths %s, L %d, route %s: %s" % (
                b.name, r, b.info["rows"][r][0] if b.info["rows"] else "-", b.lens[r, :6].tolist(), b.mins[r], route, first_candidate(want[r], got[r]))
    assert sum(len(w[0]) for w in want) > 0, (b.name, "the batch holds no candidate")
    first = sum(n for f, n in pred if f == "first"); wide = sum(n for f, n in pred if f == "wide")
    p, g, w = runs["pairwise"][1], runs["grouped"][1], runs["wide"][1]
    print(b.name, "predicted events: first form %d, wide form %d; regions" % (first, wide), {f: sum(x == f for x, _ in pred) for f in ("first", "wide", "pairwise")},
          {k: int(v) for k, v in w.items() if k.startswith("n_")})
    assert first > 0 and p["n_grouped"] == 0, (b.name, first, p["n_grouped"])
    assert g["n_grouped"] == first and g["n_grouped_wide"] == 0 and g["n_handed_back"] == -1, (b.name, first, g)
    assert w["n_grouped"] == first + wide and w["n_grouped_wide"] == wide, (b.name, first, wide, w)
    assert w["n_wide_regions"] == sum(f == "wide" for f, _ in pred), (b.name, w)
    assert w["n_handed_back"] == sum(f == "pairwise" for f, _ in pred), (b.name, w)
    if twice:
        again = G.run_routes(lib, b)
        for route in runs:
            for r in range(b.starts.shape[0]):
                assert same(runs[route][0][r], again[route][0][r]), (b.name, r, route, "a second session gives other bytes")
    return runs


def check_ends(lib, O, twice=False):
    b = batch("ends")
    assert G.window_alignments(b) == set(range(32)), sorted(set(range(32)) - G.window_alignments(b))
    last = len(b.seqs) - 1
    assert last in b.info["reversed"] and len(b.seqs[last]) % 32 != 0
    # the reverse base glen - qs - m at qs = 0 (the forward strand's window is the last of the last strand's blocks and what lies
    # behind them) and at qs + m = glen, at every width
    for g in b.info["reversed"]:
        n = len(b.seqs[g])
        assert {int(b.lens[r, g]) for r in range(len(b.mins)) if b.starts[r, g] == 0 and b.lens[r, g] > 0} >= set(G.WIDTHS), g
        assert {int(b.lens[r, g]) for r in range(len(b.mins)) if b.starts[r, g] + b.lens[r, g] == n and b.lens[r, g] > 0} >= set(G.WIDTHS), g
    assert {int(x) for x in b.lens[:, 1:].ravel()} >= {0, 1, 7, 15, 32} | set(G.WIDTHS)
    assert set(b.mins.tolist()) >= set(G.FIXED_L), sorted(set(G.FIXED_L) - set(b.mins.tolist()))
    assert [len(s) for s in b.seqs[1:]] == list(G.QLENS)
    check_batch(lib, O, b, twice)
    assert {f for f, _ in predict(O, b)} == {"first", "wide", "pairwise"}      # (the windows at L = 1 .. 3 hold more events than the first form's lists)


def check_fields(lib, O, twice=False):
    b = batch("fields")
    want = want_mums(O, b)
    nq = len(b.seqs) - 1
    for r, (what, w, L, wins) in enumerate(b.info["rows"]):
        k, lon, sp, fw = want[r]
        if what in ("whole", "poly"):      # e1 = 128; len 128 (over rep' 127 in the homopolymer)
            assert k.tolist() == [0] and lon.tolist() == [128], (what, L, k, lon)
        else:                              # spb = -127 / +127: one base, unique in the window
            assert k.tolist() == [127 if what == "minus" else 0] and lon.tolist() == [1] and L == 1, (what, k, lon)
            assert sp.tolist() == [[0 if what == "minus" else 127] * nq], (what, sp)
        assert fw.tolist() == [[0 if g in b.info["reversed"] else 1 for g in range(1, nq + 1)]]      # (a genome stored reverse-complemented holds the piece on its reverse strand)
    check_batch(lib, O, b, twice)
    assert all(f == "first" for f, _ in predict(O, b))      # (with the counts of check_batch: every region went through the grouped form)


def check_lanes(lib, O, nq, twice=False):
    b = batch("lanes%d" % nq)
    want = want_mums(O, b)
    assert (nq + 63) // 64 == {70: 2, 130: 3}[nq]
    ds = b.info["deciders"]
    assert ds == {70: [1, 63, 64, 65, 70], 130: [1, 63, 64, 65, 128, 130]}[nq]
    for x, d in enumerate(ds):      # the deciding genome decides: without it the region has other multi-MUMs
        for r in (2 * x, 2 * x + 1):
            sub = G.pieces(b, r)
            assert {len(s) for s in sub} == ({90, 40} if r % 2 == 0 else {90}) and (r % 2 or len(sub[d]) == 40)
            without = oracles.restatement_multi_mum(O, sub[:d] + sub[d + 1:], int(b.mins[r]), 1)
            assert len(want[r][0]) > 0 and (want[r][0].tolist(), want[r][1].tolist()) != (without[0].tolist(), without[1].tolist()), (nq, d, r)
    pred = predict(O, b)
    assert [f for f, _ in pred] == ["first"] * (2 * len(ds)) + ["wide"], pred
    sub = G.pieces(b, len(pred) - 1)
    assert len(set(sub[1:])) == 42 and want_events(O, sub[0], sub[-1], 3) == [(0, 0, 128, 127)]      # (40 pieces with a C, 128 x A, and 128 x T in the genomes stored reverse-complemented; rep' = 127 in the wide form's packed word)
    check_batch(lib, O, b, twice)


def check_tandem(lib, O, twice=False):
    """the restatement alone counts more events in the regions of the first grouped form than the grouped array's first capacity
    holds (3 * npairs + 64, engine_core.h): the event pass runs twice, and the candidates are the same"""
    b = batch("tandem")
    pred = predict(O, b)
    npairs = b.starts.shape[0] * (len(b.seqs) - 1)
    first = sum(n for f, n in pred if f == "first")
    assert first > 3 * npairs + 64, (first, 3 * npairs + 64)
    check_batch(lib, O, b, twice)


def test_ends_batch(libs):
    check_ends(*libs)


def test_fields_batch(libs):
    check_fields(*libs)


@pytest.mark.parametrize("nq", [70, 130])
def test_lanes_batch(libs, nq):
    check_lanes(libs[0], libs[1], nq)


def test_tandem_batch(libs):
    check_tandem(*libs)


# ------------------------------------------------------------------------------------------ the sources
def test_generator_matches_the_source():
    """the limits smallgen.py restates are those of the sources: small_pair's 128 in its three places, the 64 of the W64 choice in
    SmallPairEvents and in both grouped forms, the tables of the grouped forms"""
    eng = os.path.join(ROOT, "parsnp_amd", "csrc", "engine")
    k = open(os.path.join(eng, "kernels.h")).read(); s = open(os.path.join(eng, "store_kernels.h")).read(); e = open(os.path.join(eng, "engine_core.h")).read()
    assert re.search(r"small_pair\(int64_t nR, int64_t m\) \{ return nR <= (\d+) && m <= (\d+); \}", k).groups() == (str(G.SMALL),) * 2
    assert len(re.findall(r"if \(small_pair\(ri\.nR, m\) && !no_small\) ns = 0;", k)) == 1          # CountUnits
    assert len(re.findall(r"if \(mine && small_pair\(nR, m\) && m >= L && nR >= L &&", k)) == 1       # SmallPairEvents
    assert len(re.findall(r"if \(small_pair\(nR, ln\[g\]\) && !no_small\) ns = 0;", e)) == 1          # the host's count of the units
    assert len(re.findall(r"\bsmall_pair\(", k)) == 3 and len(re.findall(r"\bsmall_pair\(", e)) == 1 and "small_pair(" not in s.replace("(small_pair)", "")
    w64 = r"if \(nR <= (\d+) && m <= (\d+)\) (?:scan|pair_diagonals)<W64>"
    assert re.findall(w64, k) == [(str(G.WORD),) * 2] and re.findall(w64, s) == [(str(G.WORD),) * 2] * 2
    assert re.search(r"uint32_t big = nR > (\d+) \? 1u : 0u;", s).group(1) == str(G.SMALL)
    assert len(re.findall(r"if \(lens\[r \* ngen \+ g\] > %d\) big = 1;" % G.SMALL, s)) == 2
    assert int(re.search(r"#define PM_GRP_EVENTS (\d+)", s).group(1)) == G.GRP_EVENTS and "kGrpEvents = PM_GRP_EVENTS;" in s
    for name, value in (("kGrpPieces", G.GRP_PIECES), ("kWideEvents", G.WIDE_EVENTS), ("kWidePieces", G.WIDE_PIECES)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, s).group(1)) == value, name
    assert int(re.search(r"#define PM_KMAX (\d+)", k).group(1)) == G.KMAX
    assert re.search(r"c\.grp_cap = grouping \? std::max<size_t>\(grp_cap_hint, \(size_t\)npairs \* 3\) \+ 64 : 0;", e)


def test_sanitized_program(tmp_path):
    """tests/emu/pair_words_check.cpp: W64 / W128 against unsigned __int128, planes64 against the bytes at every alignment and at
    the end of the packed sequences, pair_diagonals against a naive enumeration of the maximal runs of every diagonal, the
    (first, step) split -- a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (the shifts)"""
    exe = str(tmp_path / "pair_words_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "pair_words_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and "pair_words_check ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
