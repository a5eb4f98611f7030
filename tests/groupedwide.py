"""Recursion-shaped batches with DESIGNED piece and event counts for GroupedPairEventsWide (parsnp_amd/csrc/engine/store_kernels.h),
shared by tests/test_grouped_wide.py (the kernel emulation) and tests/test_gpu_grouped_wide.py (the device).  Everything is seeded.

piece_batch   genomes of 4 kb, 16-24 regions, each a window of 64-128 bases at the same place in every genome.  Version v of the
              population carries ONE private substitution inside every window (position v // 3 of the window, the (v % 3 + 1)-th
              other base), so a batch of N versions holds exactly N distinct pieces in every region -- distinct_pieces() counts
              them from the bytes, and the tests assert the count.  Every fifth genome has the stretch [glen / 4, glen / 4 +
              glen / 3) inverted, as test_emu_engine.small_region_batch does; a window inside the stretch is requested where the
              inversion put it, and the inverted genomes draw from versions of their own (v % 5 == 4), so that a reversed piece is
              not one piece more.
event_batch   a 7-base tandem reference (small_region_batch's low_complexity): a reference window of 18-50 bases against query pieces of
              up to 128 tandem bases with a few substitutions, minsize 2-4.  Ten bases of their own at the head of every window
              and piece (the same in every genome) give the region a multi-MUM to compare; no genome is inverted here (the pieces
              are written over the tandem, an inversion of tandem around them would change nothing the search reads).  The pieces
              are found by a seeded search that counts the events of every (piece, strand) with oracles.restatement_events (an
              event counts when it is longer than rep' of its reference position) until it holds, per region, a piece whose fuller
              strand has EXACTLY the wanted count: 9 and 32 (regions the wide form takes: more than the first form's 8, within its
              own 32) and 33 (handed back; 33 events can be placed in 128 bases, so no larger count stands in for it).  How many
              such pieces exist depends on the unit (a unit that repeats inside itself has none): the tests fix the seed.
run_three     a batch through group_wide = 1, the default (the wide form is off unless asked for), group_wide = 0 and group_small = 0,
              with the counts of pm_last_timing.
sharded_batch two ranks of a sharded session (pm_session_create_sharded: the exchanges through host callbacks) on two threads.

`python groupedwide.py first LIB` runs the smallest batch in a process of its own (the GPU file's first test, under a time limit)."""
import ctypes as C
import sys
import threading
from collections import namedtuple

import numpy as np

import oracles
from seqgen import random_seq

GLEN = 4000
Batch = namedtuple("Batch", "seqs starts lens mins info")


def distinct_pieces(b):
    """per region: how many distinct query pieces (as bytes) the batch holds"""
    return [len({b.seqs[g][b.starts[r, g]:b.starts[r, g] + b.lens[r, g]] for g in range(1, len(b.seqs))}) for r in range(b.starts.shape[0])]


def _windows(rng, n_regions, lo=64, hi=128, avoid=()):
    """n_regions disjoint windows (start, length) of [8, GLEN - 8), none across a point of `avoid`"""
    out = []
    while len(out) < n_regions:
        ln = int(rng.integers(lo, hi + 1)); st = int(rng.integers(8, GLEN - 8 - ln))
        if any(st <= x < st + ln for x in avoid) or any(st < s + l + 2 and s < st + ln + 2 for s, l in out):
            continue
        out.append((st, ln))
    return out


def piece_batch(seed, nq, npieces, n_regions=16, minsize=(8, 13), zero_len=(), no_events=False):
    """nq query genomes that carry exactly `npieces` distinct pieces in every region (see the module's text; with nq < npieces the
    first nq versions of the population, one piece per genome).
    zero_len: genomes (1-based) whose piece of every third region has length 0 (one distinct piece more there).
    no_events: every window of the reference is requested 1 500 bases off, so that no piece has an event"""
    rng = np.random.default_rng(seed)
    ref = random_seq(rng, GLEN)
    a, b = GLEN // 4, GLEN // 4 + GLEN // 3
    wins = _windows(rng, n_regions, avoid=(a, b))
    assert all(3 * ln >= npieces for _, ln in wins)
    other = {65: b"CGTA", 67: b"GTAC", 71: b"TACG", 84: b"ACGT"}      # the (k + 1)-th other base
    versions = []
    for v in range(npieces):
        s = bytearray(ref)
        for st, _ in wins:
            s[st + v // 3] = other[ref[st + v // 3]][v % 3]
        versions.append(bytes(s))
    inv_v = [v for v in range(npieces) if v % 5 == 4]
    fwd_v = [v for v in range(npieces) if v % 5 != 4] if inv_v else list(range(npieces))
    seqs = [ref]; inverted = [False]
    ni = nf = 0
    for g in range(nq):
        inv = g % 5 == 4 and bool(inv_v)
        if inv:
            q = versions[inv_v[ni % len(inv_v)]]; ni += 1
            q = q[:a] + oracles.revcomp(q[a:b]) + q[b:]
        else:
            q = versions[fwd_v[nf % len(fwd_v)]]; nf += 1
        seqs.append(q); inverted.append(inv)
    assert ni >= len(inv_v) and nf >= len(fwd_v) or nq < npieces, "every version must be carried by some genome"
    starts = np.zeros((n_regions, nq + 1), np.int64); lens = np.zeros_like(starts); mins = np.zeros(n_regions, np.int32)
    for r, (st, ln) in enumerate(wins):
        for g in range(nq + 1):
            inside = inverted[g] and a <= st and st + ln <= b
            starts[r, g] = a + b - st - ln if inside else st
            lens[r, g] = ln
            if g in zero_len and r % 3 == 0:
                lens[r, g] = 0
        if no_events:
            starts[r, 0] = (st + 1500) % (GLEN - 200)
        mins[r] = int(rng.integers(minsize[0], minsize[1]))
    return Batch(seqs, starts, lens, mins, dict(npieces=npieces))


def strand_counts(O, ref_win, piece, minsize):
    """events of (piece, forward) and (piece, reverse) against the reference window, as the grouped kernels count them"""
    out = []
    for q in (piece, oracles.revcomp(piece)):
        _, _, ln, rp = oracles.restatement_events(O, ref_win, q, minsize)
        out.append(int(np.sum(ln > rp)))
    return tuple(out)


def event_batch(O, seed, wanted=(9, 32, 33, 9, 32, 33, 32, 9, 33, 32, 9, 32, 33, 9, 32, 9), nq=40):
    """one region per entry of `wanted`: its fuller (piece, strand) has exactly that many events; the other pieces of the region
    (3-5 in all) have at most 8.  info["counts"][r] = the (forward, reverse) counts of the region's pieces"""
    rng = np.random.default_rng(seed)
    unit = random_seq(rng, 7)
    ref = (unit * (GLEN // 7 + 1))[:GLEN]
    n_regions = len(wanted)
    wins = _windows(rng, n_regions, lo=128, hi=128)      # (where the query pieces go: up to 128 bases)
    seqs = [bytearray(ref) for _ in range(nq + 1)]
    starts = np.zeros((n_regions, nq + 1), np.int64); lens = np.zeros_like(starts); mins = np.zeros(n_regions, np.int32)
    counts = []

    def tandem_piece(m, nsub):
        ph = int(rng.integers(0, 7))
        p = bytearray((unit * 20)[ph:ph + m])
        for _ in range(nsub):
            p[int(rng.integers(0, m))] = b"ACGT"[int(rng.integers(0, 4))]
        return bytes(p)

    for r, (st, _) in enumerate(wins):
        word = random_seq(rng, 10)      # the same 10 bases at the head of the reference window and of every piece: the region's multi-MUM
        for q in seqs:
            q[st:st + 10] = word
        many = wanted[r] > 20      # (many events: a short reference window, the shortest minimum length, a long piece)
        for trial in range(20000):
            nR = int(rng.integers(18, 25 if many else 50)); L = 2 if many else int(rng.integers(2, 5))
            ref_win = bytes(seqs[0][st:st + nR])
            big = word + tandem_piece(int(rng.integers(60 if many else 40, 119)), int(rng.integers(0, 8)))
            c = strand_counts(O, ref_win, big, L)
            if max(c) == wanted[r]:
                break
        else:
            raise AssertionError("no piece with %d events found" % wanted[r])
        pieces = [big]; cs = [c]
        while len(pieces) < 3 + r % 3:
            p = word + tandem_piece(int(rng.integers(10, 60)), int(rng.integers(0, 3)))
            cp = strand_counts(O, ref_win, p, L)
            if max(cp) <= 8 and p not in pieces:
                pieces.append(p); cs.append(cp)
        counts.append(cs)
        mins[r] = L
        starts[r, :] = st; lens[r, 0] = nR
        for g in range(1, nq + 1):
            p = pieces[(g + r) % len(pieces)]
            seqs[g][st:st + len(p)] = p
            lens[r, g] = len(p)
    return Batch([bytes(s) for s in seqs], starts, lens, mins, dict(counts=counts, wanted=list(wanted)))


MODES = (("wide", {"group_wide": 1}), ("default", {}), ("group_wide_0", {"group_wide": 0}), ("group_small_0", {"group_small": 0}))


def run_three(lib, b):
    """{mode: (the regions' multi-MUMs, the counts of pm_last_timing)}"""
    from parsnp_amd.binding import Session
    out = {}
    for mode, tunes in MODES:
        with Session(lib, b.seqs) as s:
            for k, v in tunes.items():
                s.tune(k, v)
            got = s.multi_mum_batch(b.starts, b.lens, b.mins)
            out[mode] = (got, dict(s.last_timing()))
    return out


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4]))


def check_batch(lib, O, b):
    """the three ways agree on every region, and every fourth region is the restatement's; returns (the counts of the run with the wide form, the
    number of multi-MUMs of the checked regions)"""
    runs = run_three(lib, b)
    d = runs["wide"][0]
    n = 0
    for r in range(b.starts.shape[0]):
        for mode in ("default", "group_wide_0", "group_small_0"):
            assert same(d[r], runs[mode][0][r]), (mode, r, b.starts[r, :3], b.lens[r, :3], b.mins[r])
        if r % 4 == 0:
            sub = [b.seqs[g][b.starts[r, g]:b.starts[r, g] + b.lens[r, g]] for g in range(len(b.seqs))]
            want = oracles.restatement_multi_mum(O, sub, int(b.mins[r]), 1)
            assert same(want, d[r]), (r, b.starts[r, :3], b.lens[r, :3], b.mins[r])
            n += len(want[0])
    for mode in ("default", "group_wide_0"):      # (the wide form is off unless asked for; nobody counts the regions handed back then)
        off = runs[mode][1]
        assert off["n_grouped_wide"] == 0 and off["n_handed_back"] == -1, (mode, off)
    assert runs["default"][1]["n_grouped"] == runs["group_wide_0"][1]["n_grouped"]
    assert runs["group_small_0"][1]["n_grouped"] == 0, runs["group_small_0"][1]
    return runs["wide"][1], n


def sharded_batch(lib, b, world=2, tunes=(("group_wide", 1),)):
    """the batch on `world` ranks of a sharded session, one thread each, the two exchanges through host callbacks: every rank's
    multi-MUMs (they must be the plain session's)"""
    from parsnp_amd.binding import Session
    L = lib.L
    RED = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_int64)
    GAT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    L.pm_session_create_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int, C.c_int, RED, GAT, C.c_void_p]
    bar = threading.Barrier(world)
    box = [None] * world
    results = [None] * world

    def meet(rank, mine, combine):
        try:
            box[rank] = mine
            bar.wait(timeout=120)
            out = combine(list(box))
            bar.wait(timeout=120)
            return out
        except threading.BrokenBarrierError:
            return None

    def work(rank):
        def red(ctx, buf, count):
            mine = np.ctypeslib.as_array(buf, (max(int(count), 1),))[:count]
            out = meet(rank, mine.copy(), lambda xs: np.minimum.reduce(xs))
            if out is None:
                return 1
            mine[:] = out
            return 0

        def gat(ctx, send, nbytes, recv):
            out = meet(rank, C.string_at(send, nbytes), lambda xs: b"".join(xs))
            if out is None:
                return 1
            C.memmove(recv, out, len(out))
            return 0

        keep = (RED(red), GAT(gat))
        try:
            s = Session.__new__(Session)
            s.lib = lib; s.n = len(b.seqs); s._seqs = [bytes(x) for x in b.seqs]
            arr = (C.c_char_p * s.n)(*s._seqs); lens = (C.c_int64 * s.n)(*[len(x) for x in s._seqs])
            h = C.c_void_p()
            lib._check(L.pm_session_create_sharded(C.byref(h), -1, s.n, arr, lens, rank, world, keep[0], keep[1], None))
            s.h = h
            with s:
                for k, v in tunes:
                    s.tune(k, v)
                results[rank] = (s.multi_mum_batch(b.starts, b.lens, b.mins), dict(s.last_timing()))
        except BaseException as e:      # (the other rank must not wait for this one)
            results[rank] = e
            bar.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for x in results:
        if isinstance(x, BaseException):
            raise x
    return results


def first_batch():
    """the smallest batches: 5 query genomes drawn from a population of 33 versions (the wide form is launched and finds every
    region done), then 40 genomes that carry all 33 (the smallest batch the wide form takes)"""
    return piece_batch(3305, 5, 33, n_regions=16), piece_batch(3340, 40, 33, n_regions=16)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "first":
    from parsnp_amd.binding import Lib
    lib = Lib(sys.argv[2]); O = oracles.load_restatement()
    for b in first_batch():
        counts, n = check_batch(lib, O, b)
        print(len(b.seqs) - 1, b.info["npieces"], {k: v for k, v in counts.items() if k.startswith("n_")}, n, flush=True)
    print("first ok")
