"""Designed inputs for the SUFFIX-ARRAY path of the event search (parsnp_amd/csrc/engine/dense_kernels.h: DenseRank0, DenseKeys,
DenseHeads, DenseRerank, DenseLcp, DenseRep, SeedDense; dense_build and the re-run logic of Engine::run in engine_core.h), shared by
tests/test_dense_edges.py (the kernel emulation), tests/test_gpu_dense_edges.py (the device) and tests/emu/dense_edges_check.cpp (the
emulation as a sanitized program).  Pure Python and numpy; seeded.  The path is selected with the tunable `dense_all`: dense_all()
below sets PARSNP_TUNE for the sessions that pm_find_events opens for itself, Session.tune("dense_all", 1) does it for a session.

The naive side (no engine, no restatement): suffix_order, lcp_array, naive_rep -- rep'[l] = the longest common prefix of the suffix at
l with any other suffix of the same string, N a symbol of its own that equals itself -- and predicted_rounds.

a_references    (A) references whose rep' is read at EVERY position through one query of probes (probe_query)
round_cases     (B) one planted exact repeat of 2^r - 1, 2^r, 2^r + 1 bases, r = 1 .. 9; round_batches: the longest first / middle / last
dense_pairs     (C) designed (reference, query) pairs for SeedDense: the binary search at its ends, left-maximality at the first bases,
                the owner windows at strides 1, 2, 3 and 16, the tail rule, N; overflow_pair: more queued samples than a sub-queue holds
segment_batch, width_batches, budget_batch   (D) batches of flagged regions
calls_in_a_row  (E) the windows of six calls of one session

`python densegen.py first LIB` runs the smallest cases in a process of its own (the GPU file's first test, under a time limit)."""
import os
import sys
from collections import namedtuple

import numpy as np

from smallgen import Batch, occurrences, other, pieces, random_seq, revcomp, window_alignments  # noqa: F401  (shared with the small-region generator)

KMAX = 16                 # kMaxK: K = min(L, 16), stride = L - K + 1, minlen = K + stride - 1 = L
DENSE_MAX_LEVELS = 33     # kDenseMaxLevels
SLICES = 1024             # kSlices: sub-queues of SeedRest's queue (and of the event buffer)
UNIT_SAMPLES = 128        # kUnitSamples = 64 * kPer: query samples per work unit (a wavefront)
UNITS_PER_SLICE = 4       # SeedExtend: slice = (unit >> 2) & (kSlices - 1) -- the four wavefronts of a workgroup share a sub-queue
_SYM = bytes.maketrans(b"ACGTN", bytes(range(5)))

Pair = namedtuple("Pair", "name ref query designed Ls")          # designed: [(l, j, n, "event" | "suppressed")]
ARef = namedtuple("ARef", "name ref Ls planted floor")           # planted: [(l, repeat length)]; floor: the 5 % floor applies
Round = namedtuple("Round", "name ref query planted minsize")


def params(L):
    """(K, stride) of a minimum length: `K = minlen < kMaxK ? minlen : kMaxK, stride = minlen - K + 1` (engine_core.h)"""
    K = min(max(L, 1), KMAX)
    return K, max(L, 1) - K + 1


def queue_first_capacity(nunits):
    """a sub-queue's capacity in the first pass of a session's first call (engine_core.h, search_events; rest_cap_hint = 0)"""
    return max(nunits * UNIT_SAMPLES // 16 // SLICES, 64) + 64


def units_of(m, L):
    K, stride = params(L)
    ns = (m - K) // stride + 1 if m >= K else 0
    return (ns + UNIT_SAMPLES - 1) // UNIT_SAMPLES


class dense_all:
    """PARSNP_TUNE=dense_all=1 around the calls that open sessions of their own, restored afterwards (as indexgen.events does)"""

    def __enter__(self):
        self.old = os.environ.get("PARSNP_TUNE")
        os.environ["PARSNP_TUNE"] = "dense_all=1"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["PARSNP_TUNE"]
        else:
            os.environ["PARSNP_TUNE"] = self.old


# ------------------------------------------------------------------------------------------ the naive side
def symbols(s):
    """A C G T N as 0 .. 4 (sym_at): the engine's order of the suffixes is the order of these bytes, a suffix that ends first"""
    return bytes((c if c in b"ACGT" else ord("N")) for c in s).translate(_SYM)


def _lcp(t, a, b):
    lo, hi = 0, min(len(t) - a, len(t) - b)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if t[a:a + mid] == t[b:b + mid]:
            lo = mid
        else:
            hi = mid - 1
    return lo


def suffix_order(s):
    t = symbols(s)
    return sorted(range(len(t)), key=lambda i: t[i:])


def lcp_array(s, sa=None):
    """lcp[i] of suffix sa[i] with sa[i - 1], 0 at the first"""
    t = symbols(s)
    sa = suffix_order(s) if sa is None else sa
    return [0] + [_lcp(t, sa[i], sa[i - 1]) for i in range(1, len(sa))]


def naive_rep(s):
    sa = suffix_order(s)
    lc = lcp_array(s, sa) + [0]
    rep = [0] * len(s)
    for i, p in enumerate(sa):
        rep[p] = max(lc[i], lc[i + 1])
    return rep


def longest_repeat(s):
    return max(naive_rep(s), default=0)


def predicted_rounds(strings):
    """dense_rounds of a batch whose flagged regions are `strings`: the smallest r >= 1 with 2^r > the longest repeat of any of them
    (round k ranks the prefixes of 2^(k + 1) symbols; the sort stops when every suffix has a rank of its own; rank 0 holds the
    region, so a repeat never crosses regions); 0 when the regions hold no base"""
    if not any(len(s) for s in strings):
        return 0
    rep = max(longest_repeat(s) for s in strings)
    r = 1
    while (1 << r) <= rep:
        r += 1
    assert r < DENSE_MAX_LEVELS
    return r


def engine_rep(v, L):
    """what DenseRep stores: `v >= ri.K ? v : 0`"""
    return v if v >= params(L)[0] else 0


# ------------------------------------------------------------------------------------------ (A) rep' at every position
def _differs(c):
    return other(c) if c in b"ACGT" else ord("A")


def probe_query(ref, rep, L=1):
    """one query that shows rep' at every reference position l with l + b <= nR, b = max(rep'[l] + 1, L): per position a lead base
    that differs from ref[l - 1], ref[l : l + b], and a trailing base that differs from ref[l + b] (an N where the reference ends).
    b bases from l on are unique in the reference (b > rep'[l]), so the query suffix at the probe's body has its longest match at l
    alone, b bases long, left-maximal: the event (l, j, b), which carries rep'[l].  -> (query, {l: (j, b)})"""
    q = bytearray(); probes = {}
    n = len(ref)
    for l in range(n):
        b = max(rep[l] + 1, L)
        if l + b > n:
            continue
        q.append(_differs(ref[l - 1]) if l else ord("A"))
        probes[l] = (len(q), b)
        q += ref[l:l + b]
        q.append(_differs(ref[l + b]) if l + b < n else ord("N"))
    return bytes(q), probes


def _closed(rng, n):
    """n bases whose last is the only one of its letter: no suffix is a prefix of another, so every position can be probed"""
    last = b"ACGT"[int(rng.integers(0, 4))]
    return random_seq(rng, n - 1, bytes(c for c in b"ACGT" if c != last)) + bytes([last])


def _copy(ref, src, dst, n):
    """ref[dst : dst + n] = ref[src : src + n], an exact copy of n bases and no more (the bases before and behind differ)"""
    ref[dst:dst + n] = ref[src:src + n]
    if dst > 0 and src > 0:
        ref[dst - 1] = other(ref[src - 1])
    if dst + n < len(ref) and src + n < len(ref):
        ref[dst + n] = other(ref[src + n])


def a_references():
    """the references of (A).  Below 100 bases the last base is the only one of its letter (every position probed); from 100 on a
    reference ends in 20 random bases (a second copy that reaches the end would hide its positions: X + G + X alone exposes half)"""
    rng = np.random.default_rng(8101)
    out = []
    for n in (1, 2, 3, 31, 32, 33, 63, 64, 65):
        out.append(ARef("len%d" % n, _closed(rng, n), (1,), [], True))
    for n in (127, 128, 129, 255, 256, 257):
        out.append(ARef("len%d" % n, random_seq(rng, n), (1,), [], True))
    tail = lambda: random_seq(rng, 20)
    out.append(ARef("random", random_seq(rng, 150), (1, 8), [], True))
    out.append(ARef("tandem8", random_seq(rng, 60) + random_seq(rng, 8) * 12 + tail(), (1, 8, 17), [], True))
    out.append(ARef("homopolymer", random_seq(rng, 40) + b"A" * 70 + tail(), (1, 16), [], True))
    x = random_seq(rng, 80)
    out.append(ARef("x+g+x", x + bytes([other(x[0])]) + x + tail(), (1, 17), [], True))
    for k in (1, 2, 33):
        out.append(ARef("nrun%d" % k, random_seq(rng, 70) + b"N" * k + random_seq(rng, 60) + tail(), (1, 8), [], True))
    out.append(ARef("one_symbol", b"C" * 40, (1,), [], False))      # (rep'[l] = n - l for l > 0: only l = 0 can be probed)
    for L in (8, 16, 17):       # planted repeats of K - 1, K and K + 1 bases: `v >= ri.K ? v : 0`
        K = params(L)[0]
        for attempt in range(50):
            r = np.random.default_rng(8200 + 100 * L + attempt)
            ref = bytearray(random_seq(r, 330))
            planted = []
            for i, p in enumerate((K - 1, K, K + 1)):
                src, dst = 10 + 50 * i, 170 + 50 * i
                _copy(ref, src, dst, p)
                planted += [(src, p), (dst, p)]
            rep = naive_rep(bytes(ref))
            if all(rep[l] == p for l, p in planted):
                break
        out.append(ARef("planted%d" % L, bytes(ref), (L,), planted, True))
    return out


# ------------------------------------------------------------------------------------------ (B) rounds
ROUND_LENGTHS = tuple(sorted({(1 << r) + d for r in range(1, 10) for d in (-1, 0, 1)}))      # 1 .. 513


def _mutated(rng, s, sub):
    a = bytearray(s)
    for i in np.nonzero(rng.random(len(a)) < sub)[0]:
        if a[i] in b"ACGT":
            a[i] = other(a[i], int(rng.integers(0, 3)))
    return bytes(a)


def round_case(p):
    """a reference with one planted exact repeat of p bases in random sequence whose longest repeat, measured naively, is p (flanks
    so short that chance holds nothing longer; drawn again otherwise), and a query that is a copy with substitutions"""
    flank = 1 if p <= 1 else 3 if p <= 2 else 6 if p <= 4 else 12 if p <= 5 else 40 if p <= 9 else 120
    for attempt in range(400):
        rng = np.random.default_rng(8300 + 1000 * p + attempt)
        a, b, c = (int(x) for x in rng.integers(1, flank + 1, 3))
        ref = bytearray(random_seq(rng, a + p + b + p + c))
        _copy(ref, a, a + p + b, p)
        ref = bytes(ref)
        if longest_repeat(ref) == p:
            break
    else:
        raise AssertionError("no reference whose longest repeat is %d" % p)
    n = len(ref)
    return Round("repeat%d" % p, ref, _mutated(rng, ref, 0.03), p, max(2, min(12, n // 4)))


def _batch(name, seqs_fwd, reversed_, rows):
    """rows: (what, L, [(start, len) in forward coordinates per genome]); a genome of reversed_ is stored reverse-complemented and its
    windows are requested where that put them"""
    seqs = [revcomp(s) if g in reversed_ else s for g, s in enumerate(seqs_fwd)]
    nreg, ngen = len(rows), len(seqs)
    starts = np.zeros((nreg, ngen), np.int64); lens = np.zeros_like(starts); mins = np.zeros(nreg, np.int32)
    for r, (what, L, wins) in enumerate(rows):
        mins[r] = L
        for g, (st, ln) in enumerate(wins):
            starts[r, g] = len(seqs_fwd[g]) - st - ln if g in reversed_ else st
            lens[r, g] = ln
    return Batch(name, seqs, starts, lens, mins, dict(rows=rows, reversed=tuple(reversed_)))


def _same_windows(name, blocks, seed, sub=(0.02, 0.04), gap=0):
    """a reference that is the blocks (what, L, bases) one after another (`gap` random bases between them), two query genomes that are
    copies with substitutions, the second stored reverse-complemented; a region per block, the same window in every genome"""
    rng = np.random.default_rng(seed)
    ref = b""; rows = []
    for what, L, s in blocks:
        rows.append((what, L, [(len(ref), len(s))] * 3))
        ref += s + random_seq(rng, gap)
    fwd = [ref] + [_mutated(rng, ref, x) for x in sub]
    return _batch(name, fwd, (2,), rows)


def round_batches():
    """{name: (batch, index of the region with the longest repeat)}: a region with a planted repeat of 40 bases (6 rounds) first, in
    the middle and last among regions of 2 .. 4 rounds, and a batch whose regions are all told apart after one round"""
    out = {}
    rng = np.random.default_rng(8400)
    long_one = round_case(40).ref
    short = [round_case(p).ref for p in (2, 3, 5, 9, 4, 7)]
    for where, at in (("first", 0), ("middle", 3), ("last", 6)):
        blocks = [("short", 5, s) for s in short]
        blocks.insert(at, ("long", 9, long_one))
        out["longest_" + where] = (_same_windows("longest_" + where, blocks, 8410 + at, gap=3), at)
    ones = []
    while len(ones) < 9:       # no two-base repeat: 2^1 > the longest repeat of 0 or 1
        s = random_seq(rng, int(rng.integers(2, 8)))
        if longest_repeat(s) <= 1:
            ones.append(s)
    out["one_round"] = (_same_windows("one_round", [("one", 2, s) for s in ones], 8420, gap=2), None)
    return out


# ------------------------------------------------------------------------------------------ (C) SeedDense
def _pair(rng, nR, m, alphabet=b"ACGT"):
    return bytearray(random_seq(rng, nR, alphabet)), bytearray(random_seq(rng, m, alphabet))


def _put(ref, q, l, j, n):
    """the query holds ref[l : l + n] at j, bounded by differing bases where both sides have room"""
    q[j:j + n] = ref[l:l + n]
    if l > 0 and j > 0:
        q[j - 1] = _differs(ref[l - 1])
    if l + n < len(ref) and j + n < len(q):
        q[j + n] = _differs(ref[l + n])


def dense_pairs():
    """{name: Pair}: the designed pairs of (C).  A stretch that has to come out of SeedDense has a decoy in the reference -- a copy of
    its first bases, 20 or as many as its owners' K-mers need -- so that its samples' K-mers occur twice and are queued, while the
    stretch itself is longer than the copy and unique"""
    out = {}
    rng = np.random.default_rng(8500)

    def add(name, ref, q, designed, Ls):
        out[name] = Pair(name, bytes(ref), bytes(q), designed, tuple(Ls))

    # -- the query suffix against the reference's suffixes
    ref, q = _pair(rng, 200, 170, b"CGT")          # below every reference suffix, and a proper prefix of the smallest (c == qlen)
    ref[70:100] = b"AAAAAA" + random_seq(rng, 24, b"CGT")
    _put(ref, q, 70, 150, 20)
    add("order/below_all", ref, q, [(70, 150, 20, "event")], (12, 17, 20, 21))
    ref, q = _pair(rng, 200, 161, b"ACG")          # above every one: the match goes on with a T where the largest suffix holds less
    ref[70:100] = b"TTTTTT" + random_seq(rng, 24, b"ACG")
    _put(ref, q, 70, 100, 20); q[120] = ord("T")
    add("order/above_all", ref, q, [(70, 100, 20, "event")], (12, 17, 20, 21))
    ref, q = _pair(rng, 200, 130)                  # equal to a whole reference suffix (c == rlen)
    _copy(ref, 175, 40, 20)
    _put(ref, q, 175, 60, 25)
    add("order/whole_suffix", ref, q, [(175, 60, 25, "event")], (8, 17, 25, 26))
    ref, q = _pair(rng, 200, 130)                  # a proper prefix of one (c == qlen)
    _copy(ref, 50, 120, 20)
    _put(ref, q, 50, 105, 25)
    add("order/proper_prefix", ref, q, [(50, 105, 25, "event")], (8, 17, 25, 26))
    ref, q = _pair(rng, 200, 130)                  # both at once: the two sequences end together
    _copy(ref, 175, 40, 20)
    _put(ref, q, 175, 105, 25)
    add("order/both_ends", ref, q, [(175, 105, 25, "event")], (8, 17, 25, 26))
    ref, q = _pair(rng, 240, 160)                  # the two SA neighbours share equally much with the query (llo == lhi): W is held twice
    w = random_seq(rng, 14)
    ref[80:95] = w + b"A"; ref[160:175] = w + b"G"; ref[79] = ord("A"); ref[159] = ord("C")
    q[70:86] = b"G" + w + b"C"
    _copy(ref, 10, 200, 20)
    _put(ref, q, 10, 120, 25)                      # (an ordinary stretch beside it: the case holds an event)
    add("order/tie", ref, q, [(80, 71, 14, "suppressed"), (10, 120, 25, "event")], (8, 12, 14))
    # -- left-maximality at the first bases
    for name, l, j in (("j0_zero", 60, 0), ("l0_zero", 0, 50), ("both_zero", 0, 0)):
        ref, q = _pair(rng, 220, 180)
        _copy(ref, l, 130, 20)
        _put(ref, q, l, j, 30)
        add("left/" + name, ref, q, [(l, j, 30, "event")], (8, 16, 17, 19))
    # -- uniqueness: the copy alone (ms == rep': suppressed) and with one more base (rep' + 1: reported), inside a long match
    ref = bytearray(random_seq(rng, 400))
    _copy(ref, 60, 260, 40)
    q = bytearray(ref[:200]) + bytearray(b"N") + ref[60:100] + bytearray(b"N") + ref[60:101] + bytearray(b"N")
    q[30] = other(q[30])
    add("unique/copy", ref, q, [(60, 201, 40, "suppressed"), (60, 242, 41, "event")], (8, 17, 31, 40, 41))
    # -- the owner windows: left ends 0 .. stride - 1 bases before a queued sample's K-mer, and exactly stride before it
    for L in (16, 17, 18, 31):
        K, stride = params(L)
        n, dec = K + 3 * stride + 2, K + 2 * stride
        count = stride + 2
        half = 10 + count * (n + 3)
        ref = bytearray(random_seq(rng, half + count * (dec + 3) + 30))
        q = bytearray(); designed = []
        for i in range(count):
            l = 5 + i * (n + 3)
            _copy(ref, l, half + i * (dec + 3), dec)
            if i == 0:
                j = 0                                                        # the piece's first base (the `j0 >= 0` clamp)
            else:
                d = i - 1                                                    # the left end lies d bases before a sample
                j = len(q) + 2
                while (-j) % stride != d % stride:
                    j += 1
                q += random_seq(rng, j - len(q))
            q += bytes(n) + b"A"
            designed.append((l, j, n, "event"))
        q += random_seq(rng, 40)
        for l, j, n, _ in designed:
            _put(ref, q, l, j, n)
        add("owner/stride%d" % stride, ref, q, designed, (L,))
    # -- the tail rule: a stretch that ends on the query's last base with m - j0 = minlen - 1, minlen, minlen + 1; the K-mer of the
    #    sample that owns it is held twice (at stride 1 that is the whole stretch of minlen bases: ms == rep', suppressed)
    for L in (8, 17, 19):
        K, stride = params(L)
        for dt in (-1, 0, 1):
            t = L + dt
            ref, q = _pair(rng, 260, 140 + t)
            j0 = len(q) - t
            off = (-j0) % stride
            _copy(ref, 40 + off, 120, K)
            _put(ref, q, 40, j0, t)
            _copy(ref, 150, 210, 20)
            _put(ref, q, 150, 20, 30)                  # (an ordinary stretch beside it: the case holds an event at minlen - 1 too)
            kind = "event" if (t > K if off == 0 else True) else "suppressed"
            add("tail/%d%+d" % (L, dt), ref, q, [(40, j0, t, kind), (150, 20, 30, "event")], (L,))
    # -- N: in the query inside a stretch (two events), on both sides at the same place (N equals N: one event)
    ref, q = _pair(rng, 260, 200)
    _copy(ref, 50, 170, 20); _copy(ref, 81, 200, 20)
    _put(ref, q, 50, 60, 60); q[90] = ord("N")
    add("n/query", ref, q, [(50, 60, 30, "event"), (81, 91, 29, "event")], (8, 17, 29, 30))
    ref, q = _pair(rng, 260, 200)
    ref[80:83] = b"NNN"
    _copy(ref, 50, 170, 20)
    _put(ref, q, 50, 60, 60)
    add("n/both", ref, q, [(50, 60, 60, "event")], (8, 17, 60))
    return out


PAIR_FAMILIES = ("order", "left", "unique", "owner", "tail", "n")


def overflow_pair():
    """(reference, queries, L): one 2 000-base string twice, the second copy with a substitution every 50 bases -- nearly every K-mer
    is shared, so nearly every sample of the queries (copies with a few substitutions) is queued, and a match of more than 99 bases
    is still unique in the reference (with two exact copies no match is, and the expected list is empty)"""
    rng = np.random.default_rng(8600)
    x = random_seq(rng, 2000)
    y = bytearray(x)
    for i in range(25, 2000, 50):
        y[i] = other(y[i])
    return x + bytes(y), [_mutated(rng, x + random_seq(rng, 300), 0.004), revcomp(_mutated(rng, x, 0.008))], 12


# ------------------------------------------------------------------------------------------ (D) segments
def segment_batch():
    """the shapes of (D) in one batch: regions of 0 bases first, in the middle and last; the same 150 bases as two adjacent regions
    and a third apart; three neighbouring regions cut out of one tandem array of period 8 (a suffix of one would go on into the next);
    regions of 1 base; 32 regions of 33 bases one after another (every ref_pos & 31); and `left_edge`: a query piece that begins 7
    bases into its window right behind a base equal to the reference's (the match is cut by the piece's first base: j0 = 0, l0 = 7);
    and `keys/prefix` (below)"""
    rng = np.random.default_rng(8700)
    t = random_seq(rng, 150)
    unit = random_seq(rng, 8)
    edge = bytearray(random_seq(rng, 170)); _copy(edge, 7, 100, 20)
    # `keys/prefix`: the region ENDS with Y, a copy of 20 bases it holds before (there followed by Z), and is not the last region: the
    # suffix Y ends before its second key half and must sort BEFORE Y + Z (second = 0), not by what the next region begins with; the
    # query pieces hold Y + Z[:5] + T with T above Z[5], so the search comes past both suffixes
    y, z = random_seq(rng, 20), random_seq(rng, 20, b"ACG")
    prefix = random_seq(rng, 40) + y + z + random_seq(rng, 60) + y
    prefix_q = [random_seq(rng, 60) + y + z[:5] + b"T" + random_seq(rng, 74) for _ in range(2)]
    blocks = [("zero/first", 8, b""), ("same/adjacent0", 12, t), ("same/adjacent1", 12, t), ("spacer", 9, random_seq(rng, 41)),
              ("tandem/0", 10, unit * 20), ("tandem/1", 10, unit * 20), ("tandem/2", 10, unit * 20), ("zero/middle", 8, b""),
              ("one/0", 1, random_seq(rng, 1)), ("one/1", 1, random_seq(rng, 1)), ("same/apart", 12, t), ("left_edge", 12, bytes(edge)),
              ("keys/prefix", 12, prefix)]
    blocks += [("align/%d" % i, 9, random_seq(rng, 33)) for i in range(32)]
    blocks += [("zero/last", 8, b"")]
    ref = b""; rows = []
    for what, L, s in blocks:
        rows.append([what, L, [(len(ref), len(s))] * 3])
        ref += s
    fwd = [ref, _mutated(rng, ref, 0.02), _mutated(rng, ref, 0.04)]
    for r, (what, L, wins) in enumerate(rows):
        if what == "left_edge":
            st, ln = wins[0]
            fwd[1] = fwd[1][:st] + ref[st:st + ln] + fwd[1][st + ln:]; fwd[2] = fwd[2][:st] + ref[st:st + ln] + fwd[2][st + ln:]
            rows[r][2] = [(st, ln), (st + 7, ln - 7), (st + 7, ln - 7)]
        if what == "keys/prefix":
            st, ln = wins[0]
            for g in (1, 2):
                fwd[g] = fwd[g][:st] + prefix_q[g - 1] + fwd[g][st + ln:]
    return _batch("segments", fwd, (2,), [tuple(x) for x in rows])


WIDTHS = ((13, 255), (13, 256), (13, 257), (205, 1023), (205, 1024), (205, 1025))      # (flagged regions, dense length n)


def width_batch(nflag, n):
    """nflag regions one after another, n bases together, the last one with an N: round 0's largest rank is 5 * nflag - 1 (64 and
    1 024: one bit more than 5 * nflag - 2 needs), and every later round ranks up to n - 1"""
    rng = np.random.default_rng(8800 + n)
    lens = [n // nflag + (1 if i < n % nflag else 0) for i in range(nflag)]
    blocks = [("w%d" % i, 3 if ln < 10 else 6, random_seq(rng, ln)) for i, ln in enumerate(lens)]
    what, L, s = blocks[-1]
    blocks[-1] = (what, L, s[:-2] + b"N" + s[-1:])
    return _same_windows("width%dx%d" % (nflag, n), blocks, 8900 + n, sub=(0.05, 0.08))


def budget_batch():
    """a batch shaped like the recursion's, 41 regions, with a tandem array of 500 copies in region 0, in region 20 and in the last
    one, for a work budget of 48: those regions run out of budget and take the path, the others walk"""
    rng = np.random.default_rng(8950)
    unit = b"ACGTTGCA"
    blocks = [("plain", int(rng.integers(9, 21)), random_seq(rng, int(rng.integers(20, 400)))) for _ in range(41)]
    for at in (0, 20, 40):
        blocks[at] = ("array", 12, random_seq(rng, 90) + unit * 500 + random_seq(rng, 90))
    return _same_windows("budget", blocks, 8960, sub=(0.02, 0.05))


# ------------------------------------------------------------------------------------------ (E) calls in a row
def calls_in_a_row():
    """(genomes, calls): calls = [(name, starts, lens, mins)] over ONE set of genomes -- a window with a planted repeat of 300 bases (9
    rounds), a window of 2 rounds, the first again, 11 regions, 2 regions, the 11 again"""
    rng = np.random.default_rng(9000)
    big = round_case(300).ref
    small = round_case(3).ref
    parts = [big, small] + [random_seq(rng, int(rng.integers(40, 160))) for _ in range(11)]
    at = [0]
    for p in parts:
        at.append(at[-1] + len(p))
    ref = b"".join(parts)
    seqs = [ref, _mutated(rng, ref, 0.02), _mutated(rng, ref, 0.04)]

    def call(name, idx, L):
        st = np.array([[at[i]] * 3 for i in idx], np.int64); ln = np.array([[len(parts[i])] * 3 for i in idx], np.int64)
        return (name, st, ln, np.array([L] * len(idx), np.int32))
    nine, two = call("nine_rounds", [0], 11), call("two_rounds", [1], 2)
    eleven, pair_ = call("eleven_regions", list(range(2, 13)), 9), call("two_regions", [5, 0], 10)
    return seqs, [nine, two, nine, eleven, pair_, eleven]


def smaller_after_larger():
    """(genomes, calls, designed): a call over a region of 300 bases of a tandem (every LCP large, every level's ranks written), then a
    call over a region of 200 bases -- the buffers are kept, so element 200 of every rank array and of lcp[] still holds the first
    call's value.  The second region ends with Y, 16 bases it holds before, there followed by c = the base at 200 of the FIRST
    region: dense_lcp without its `end` bound reads the first call's rank at 200 on level 0, finds c, and makes Y + c a repeat of 17
    bases, which suppresses the designed multi-MUM (60, 17).  The region's largest suffix begins at its one N (symbol 4): DenseRep
    reading lcp[t + 1] past the segment gives that position the first call's LCP, which suppresses the designed multi-MUM (120, 30)"""
    rng = np.random.default_rng(9100)
    while True:         # (SA position 200 of the tandem inside a block of equal phases, not on the border of two)
        w1 = (random_seq(rng, 9) * 40)[:300]
        if lcp_array(w1)[200] >= 30:
            break
    y = random_seq(rng, 16)
    w2 = bytearray(random_seq(rng, 60) + y + w1[200:201] + random_seq(rng, 43) + b"N" + random_seq(rng, 63) + y)
    w2[59] = other(w2[183])                     # (Y is a copy of 16 bases and no more)
    assert len(w2) == 200
    ref = w1 + bytes(w2)
    qs = []
    for g in range(2):
        q = bytearray(ref)
        for at in (59, 77, 119, 150):
            q[300 + at] = other(q[300 + at], g)
        q[100] = other(q[100], g)
        qs.append(bytes(q))
    call = lambda st, ln: (np.array([[st] * 3], np.int64), np.array([[ln] * 3], np.int64), np.array([12], np.int32))
    return [ref] + qs, [call(0, 300), call(300, 200)], [(60, 17), (120, 30)]


# ------------------------------------------------------------------------------------------ the case file of the sanitized program
def write_cases(path, O, pair_records, batches):
    """the cases for tests/emu/dense_edges_check.cpp.  pair_records: [(name, ref, query, L, strand, sorted (l, j, len, rep'))] -- the
    restatement's events as the tests compare them; batches: [(Batch, the restatement's multi-MUMs per region)]"""
    with open(path, "w") as f:
        for name, ref, q, L, strand, ev in pair_records:
            f.write("PAIR %s %d %d %d\n%s\n%s\n" % (name.replace(" ", "_"), L, strand, len(ev), ref.decode(), q.decode()))
            for e in ev:
                f.write("%d %d %d %d\n" % e)
        for b, want in batches:
            nreg, ngen = b.starts.shape
            f.write("BATCH %s %d %d\n" % (b.name, ngen, nreg))
            for s in b.seqs:
                f.write(s.decode() + "\n")
            for r in range(nreg):
                k, lon, sp, fw = want[r][:4]
                f.write("%d %s %s %d\n" % (b.mins[r], " ".join(map(str, b.starts[r])), " ".join(map(str, b.lens[r])), len(k)))
                for c in range(len(k)):
                    f.write("%d %d %s %s\n" % (k[c], lon[c], " ".join(map(str, sp[c])), " ".join(map(str, fw[c]))))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "first":
    import oracles
    from parsnp_amd.binding import Lib, Session
    lib = Lib(sys.argv[2]); O = oracles.load_restatement()
    for a in a_references()[:3]:          # references of 1, 2 and 3 bases, rep' at every position
        rep = naive_rep(a.ref)
        q, probes = probe_query(a.ref, rep, 1)
        with dense_all():
            j, l, n, r = lib.find_events(a.ref, q, 1, 0)
        got = sorted(zip(l.tolist(), j.tolist(), n.tolist(), r.tolist()))
        for p, (at, b) in probes.items():
            assert (p, at, b, rep[p]) in got, (a.name, p, got)
    c = round_case(1)
    with Session(lib, [c.ref, c.query]) as s:
        s.tune("dense_all", 1)
        got = s.whole(c.minsize)
        t = dict(s.last_timing())
    want = oracles.restatement_multi_mum(O, [c.ref, c.query], c.minsize, 1)
    assert all(np.array_equal(x, y) for x, y in zip(want[:4], got[:4])), c.name
    assert t["dense_regions"] == 1 and t["dense_rounds"] == predicted_rounds([c.ref]), t
    print("first ok")
