"""Seeded generator of DESIGNED (reference, query) pairs for the event search (parsnp_amd/csrc/engine/kernels.h: SeedExtend, SeedRest,
EventBucketCount / EventPlace / EventOrder, the wavefront scan): exact stretches whose lengths are the ones at which the device
bodies change path, with one difference of a chosen kind after each.  Test infrastructure only; the checks and the floors that
prove a case still holds what it was designed to hold are in tests/test_search_edges.py.

The numbers below restate the defaults of kernels.h (PM_PER, PM_LEAD, PM_KMAX, PM_WAVE_EVENTS); test_search_edges.py compares them
with the header, so a changed default turns that test red instead of leaving the lengths beside the edges."""
import numpy as np

import oracles
from oracles import revcomp
from seqgen import random_seq

KPER = 2            # kPer: adjacent query samples of a SeedExtend lane
KLEAD = 4           # kLead: one lane in kLead probes the index for the others
KMAX = 16           # kMaxK: longest seed
WAVE_EVENTS = 512   # kWaveEvents: events per wavefront of the scan
BLOCK = 256         # kChunkPos: reference positions per bucket of the event order
SMALL = 128         # small_pair(): both sides at most this long -> SmallPairEvents, no SeedExtend
MAX_STRETCH = 5000  # the restatement spends ~ len^2 log n / 2 byte compares on a match: longer designed stretches are left out

MINSIZES = (8, 16, 17, 19, 25, 31, 32, 48, 90)      # strides 1, 1, 2, 4, 10, 16 (windows, `follow`), 17, 33, 75 (tags from memory)
ALPHA = b"ACGT"


def params(minsize):
    """(K, stride, own, unit): seed length, sampling step, bases of the query a lane owns, bases a unit (wavefront) owns"""
    K = min(minsize, KMAX)
    stride = minsize - K + 1
    return K, stride, KPER * stride, 64 * KPER * stride


def windows(minsize):
    """SeedExtend's `regs`: all K-mers of a lane start inside one 32-base window; with stride <= K this is `follow` for a query
    piece of at least one unit"""
    K, stride, _, _ = params(minsize)
    return (KPER - 1) * stride + K <= 32 and stride <= K


def next_base(c):
    return ALPHA[(ALPHA.index(c) + 1) % 4]


def other_base(*avoid):
    return next(c for c in ALPHA if c not in avoid)


def edge_lengths(minsize):
    """(lengths, unit-sized lengths) of the stretches: see the module text of test_search_edges.py for what each one pins.
    The window-edge values are planted as arm lengths (64 - K - u * stride: bases after the K-mer) and as whole stretches
    (64 - u * stride: the K-mer at the stretch's start included) -- which of the two ends on the edge depends on where the
    stretch starts in its lane, and planted(..., phase=) puts the start on a lane's sample."""
    K, stride, own, unit = params(minsize)
    out = [minsize - 1, minsize, minsize + 1]
    for d in (0, stride):
        out += [64 - K - 1 - d, 64 - K - d, 64 - K + 1 - d, 64 - 1 - d, 64 - d, 64 + 1 - d]
    out += [31, 32, 33, 63, 64, 65, 95, 96, 97, own - 1, own, own + 1]
    big = [unit - 1, unit, unit + 1, 128 * stride + 40, 128 * stride + 70]      # (+ 70: past lane 63's windows at every stride <= 16)
    seen, small = set(), []
    for x in out:
        if x > 0 and x not in seen:
            seen.add(x); small.append(x)
    return small, [x for x in big if x <= MAX_STRETCH]


class Planted:
    """query + what was planted: recs = (reference start, query start, true length, kind of the difference after it, designed length
    or 0 for a filler) -- the true length is measured on the finished query along the stretch's diagonal, so a deletion whose
    skipped base equals its neighbour (the stretch runs one base further) is accounted for"""

    def __init__(self, ref, query, recs):
        self.ref, self.query, self.recs = ref, query, recs


def _true_extent(ref, q, rs, qs, L):
    a = 0
    while rs - a > 0 and qs - a > 0 and ref[rs - a - 1] == q[qs - a - 1]:
        a += 1
    b = L
    while rs + b < len(ref) and qs + b < len(q) and ref[rs + b] == q[qs + b]:
        b += 1
    return rs - a, qs - a, a + b


def planted(ref, lengths, kinds, own=0, phase=None, unit=0, unit_aligned=(), cycle=True, last_open=False, exact=()):
    """a query that copies `ref` in exact stretches of the listed lengths (cycled while the reference lasts), each followed by one
    difference of the listed kinds (cycled): sub = the next base of the alphabet, ins = one extra query base, del = one reference
    base skipped, n = an N in the query.
    phase (with own): a filler stretch ending in a substitution goes before every designed stretch so that it starts at query offset
    = phase (mod own) -- on the lane's sample phase / stride; the lengths in unit_aligned start at offset = phase (mod unit), a
    wavefront's first lane.  last_open: no difference after the last stretch (the match ends with the query).  exact: lengths
    that get a substitution on either side, whatever the rotation says (a deletion beside a stretch can lengthen it)."""
    q = bytearray(); recs = []; r = 0; i = 0

    def put(L, kind, designed, closing=True):
        nonlocal r
        qs = len(q); rs = r
        q.extend(ref[r:r + L]); r += L
        if not closing:
            pass
        elif kind == "sub":
            q.append(next_base(ref[r])); r += 1
        elif kind == "n":
            q.append(ord("N")); r += 1
        elif kind == "ins":
            q.append(other_base(ref[r - 1], ref[r]))
        elif kind == "del":
            r += 1
        else:
            raise ValueError(kind)
        recs.append([rs, qs, L, kind if closing else "end", designed])

    while True:
        if i >= len(lengths) and not cycle:
            break
        L = lengths[i % len(lengths)]; kind = kinds[i % len(kinds)]
        if L in exact or lengths[(i + 1) % len(lengths)] in exact:
            kind = "sub"
        mod = unit if (unit and L in unit_aligned) else (own if phase is not None else 0)
        fill = 0
        if mod and len(q) % mod != (phase or 0) % mod:      # (fill + the substitution after it) bases up to the wanted offset
            fill = ((phase or 0) - len(q) - 1) % mod
            if fill == 0:
                fill = mod
        if r + fill + 1 + L + 2 > len(ref):
            break
        if fill > 0:
            put(fill, "sub", 0)
        last = last_open and not cycle and i == len(lengths) - 1
        put(L, kind, L, closing=not last)
        i += 1
    query = bytes(q)
    out = []
    for rs, qs, L, kind, designed in recs:
        a, b, n = _true_extent(ref, query, rs, qs, L)
        out.append((a, b, n, kind, designed))
    return Planted(ref, query, out)


def needed(lengths, own=0, unit=0, unit_aligned=()):
    return sum(lengths) + len(lengths) * (2 + own) + len([x for x in lengths if x in unit_aligned]) * unit + 8


# ------------------------------------------------------------------------------------------ the designed pairs
def edge_pairs(minsize, seed=0):
    """{name: Planted}: every length of edge_lengths(minsize) with substitutions only and with the sub / ins / del / N mix (the
    short lengths twice there: five kinds in rotation, so a length meets two of them), and -- where the lanes hold windows -- once
    starting on a lane's sample 0 and once on its sample 1"""
    K, stride, own, unit = params(minsize)
    small, big = edge_lengths(minsize)
    rng = np.random.default_rng(1000 * minsize + seed)
    out = {}
    win = windows(minsize)
    aligned = tuple(big) if win else ()      # (without windows the lanes form no runs: nothing ends with the unit)
    variants = [("sub", ("sub",), None), ("mix", ("sub", "ins", "del", "n", "sub"), None)]
    if win:
        variants += [("sample0", ("sub",), 0), ("sample1", ("sub", "n"), stride % own)]
    for name, kinds, phase in variants:
        ls = small * (2 if name == "mix" else 1) + big
        ref = random_seq(rng, needed(ls, own if phase is not None else 0, unit, aligned) + 40)
        out[name] = planted(ref, ls, kinds, own=own, phase=phase, unit=unit if win else 0, unit_aligned=aligned, cycle=False)
    return out


LONG_ARMS = (2047, 2048, 2049, 4095, 4096, 4097, 4500)


def _around(rng, head, tail, minsize):
    """stretch lengths of ordinary divergence that fill `head` bases before and `tail` bases after a long stretch"""
    def fill(room):
        out, s = [], 0
        while True:
            x = int(rng.integers(minsize, minsize + 60))
            if s + x + 1 > room:
                return out
            out.append(x); s += x + 1
    return fill(head), fill(tail)


def long_arm_pairs(minsize, seed=0):
    """{name: Planted}: a stretch 700 + L + 300 for L in LONG_ARMS (two or three stretches per pair, so that a sequence stays under
    20 kb): the arm outruns its wavefront's windows and is finished from memory -- on the device by the whole wavefront, 32 bases
    per lane and 64 * 32 per round.  Where the lanes hold windows, also stretches that start on a wavefront's first lane and end
    t bases after the point where that loop takes over (offset 63 * own + 64 of the unit), t = 0, 31, 32, 2047, 2048: the
    difference in lane chunk 0 (first and last base), 1 and 63 of round 0 and in chunk 0 of round 1."""
    K, stride, own, unit = params(minsize)
    rng = np.random.default_rng(2000 * minsize + seed)
    out = {}
    groups = [LONG_ARMS[0:3], LONG_ARMS[3:5], LONG_ARMS[5:7]]
    for gi, group in enumerate(groups):
        ls = []
        for L in group:
            pre, post = _around(rng, 700, 300, minsize)
            ls += pre + [L] + post
        ref = random_seq(rng, needed(ls) + 40)
        out["long%d" % gi] = planted(ref, ls, ("sub", "sub", "ins", "n", "del"), cycle=False, exact=LONG_ARMS)
    if windows(minsize):
        takeover = 63 * own + 64
        for name, ts in (("chunks0", (0, 31, 32)), ("chunks1", (2047, 2048))):
            ls = [takeover + t for t in ts]
            ref = random_seq(rng, needed(ls, own, unit, ls) + 40)
            out[name] = planted(ref, ls, ("sub", "n"), own=own, phase=0, unit=unit, unit_aligned=tuple(ls), cycle=False)
    return out


def clamp_pairs(minsize, seed=0):
    """{name: (ref, query)}: the match that ends on the last base of the shorter side (`f_maxr`) or starts on its first (`lim` of
    the left arm), and query pieces of m = 128 * stride * k + r bases (the last unit holds one lane; its sample 1 is past the
    piece; at k = 1 `follow` switches)"""
    K, stride, own, unit = params(minsize)
    rng = np.random.default_rng(3000 * minsize + seed)
    base = [minsize + 3, 70, 150, 5 * own + 1, 40, 2 * minsize, 33]
    n = 2 * unit + K + stride + 600
    ref = random_seq(rng, n + 64)
    p = planted(ref, base, ("sub", "sub", "n"))
    q = bytearray(p.query)
    for k in (1, 2):      # (substitutions and N only: the query lies on diagonal 0) every cut below falls inside an exact stretch
        a, b = unit * k - minsize - 10, unit * k + K + stride + 10
        q[a:b] = ref[a:b]
    q = bytes(q)
    out = {}
    # the query a prefix of the reference's design, ending inside a stretch of >= 300 exact bases (an arm from memory meets the end)
    tail = planted(ref, [90, 61, 300 + minsize], ("sub",), cycle=False, last_open=True)
    out["query_is_prefix"] = (ref, tail.query)
    out["reference_is_prefix"] = (ref[:len(tail.query)], tail.query + ref[len(tail.query):len(tail.query) + 200])
    exact = ref[:max(2 * unit, 400)]      # (no difference at all: one match, both sides end together)
    out["identical"] = (exact, exact)
    for e in sorted({1, K - 1, K, K + stride}):
        extra = random_seq(rng, e)
        out["front%d" % e] = (ref, extra + q)              # the first match starts on the reference's first base ...
        out["rfront%d" % e] = (extra + ref, q)             # ... and on the query's
    for k in (1, 2):
        for r in sorted({-1, 0, 1, K - 1, K, K + stride - 1, K + stride}):
            m = unit * k + r
            out["m%dx+%d" % (k, r)] = (ref, q[:m])
    return out


def leader_pairs(minsize, seed=0):
    """{name: (ref, query, positions)} for the minimum lengths whose lanes follow a leader: a substitution (or an insertion) inside
    the K-mer of a leader's first sample -- lane 0, a lane in the middle and lane 64 - kLead of a wavefront -- and no other
    difference for 2 * kLead lanes on either side: the followers take the leader before, the leader after, or their own probe"""
    K, stride, own, unit = params(minsize)
    assert windows(minsize)
    rng = np.random.default_rng(4000 * minsize + seed)
    quiet = 2 * KLEAD * own + 64 + K
    ref = random_seq(rng, 5 * unit + 300)
    out = {}

    def build(spots, insert):
        q = bytearray(ref)
        marks = sorted(spots)
        x = 37
        while x < len(ref) - 2:      # ordinary differences elsewhere (so that the matches stay short for the restatement)
            if all(abs(x - s) > quiet for s in marks):
                q[x] = next_base(q[x])
            x += 211 + (x % 97)
        for s in sorted(marks, reverse=True):
            if insert:
                q[s:s] = bytes([other_base(ref[s - 1], ref[s])])
            else:
                q[s] = next_base(ref[s])
        return bytes(q)

    lanes = (0, 32 // KLEAD * KLEAD, 64 - KLEAD)
    spots = [(u + 1) * unit + lane * own + K // 2 for u, lane in enumerate(lanes)]      # lane `lane` of wavefront u + 1
    out["leaders_sub"] = (ref, build(spots, False), spots)
    for s, lane in zip(spots, lanes):
        out["leader%d_ins" % lane] = (ref, build([s], True), [s])
    return out


def repeat_pair(minsize, seed=0):
    """(ref, query, info): a 40-base (or minsize + 8) stretch of the reference copied 1 kb further on, inside a long match (shared
    K-mers: followers probe for themselves, kMulti slots and chains); the stretch alone between two N (len == rep': suppressed) and
    with one more base (len == rep' + 1: reported); a palindromic K-mer on a sampled offset (seeds both strands)"""
    K, stride, own, unit = params(minsize)
    rng = np.random.default_rng(5000 * minsize + seed)
    R = max(40, minsize + 8)
    n = max(3000, 2 * unit + 2200)
    ref = bytearray(random_seq(rng, n))
    a, b = 500, 1500 + R
    ref[b:b + R] = ref[a:a + R]
    ref[b - 1] = other_base(ref[a - 1]); ref[b + R] = other_base(ref[a + R])      # the copy is exactly R bases
    pal_at = (2000 // stride) * stride
    half = random_seq(rng, K // 2)
    ref[pal_at:pal_at + K] = half + revcomp(half)
    ref = bytes(ref)
    q = bytearray(ref)
    for x in range(300, n - 2, 389):      # a few ordinary differences, none inside the copies or the palindrome
        if not (a - 60 <= x <= a + R + 60 or b - 60 <= x <= b + R + 60 or pal_at - 60 <= x <= pal_at + K + 60):
            q[x] = next_base(q[x])
    body = bytes(q)
    alone = ref[a:a + R]
    query = body + b"N" + alone + b"N" + ref[a:a + R + 1] + b"N"
    info = {"a": a, "b": b, "R": R, "j_alone": len(body) + 1, "j_plus1": len(body) + 1 + R + 1, "pal_at": pal_at}
    return ref, query, info


# ------------------------------------------------------------------------------------------ multi-genome sets
BUCKET_PLAN = (0, 1, 2, 3, 8, 9, 28, 4, 5, 6, 7, 10, 0, 28, 3, 8, 2, 9, 1, 28, 6, 7, 0, 5, 6, 7, 8, 0, 1, 4)      # intended events per consecutive 256-position block


def bucket_set(seed=0):
    """(seqs, minsize, plan, edge starts): minsize 8; the queries are N (at this length any base sequence holds dozens of chance
    8-mers per block) but for planted stretches of 8 and 9 bases, `plan[b]` of them starting in block b of the reference -- the branches of EventOrder (0, 1, 2, 3..8 in registers,
    more by Shell's gaps); stretches that start on positions 255, 256 and 257 (mod 256): the heads of the bucket runs fall inside
    a wavefront of EventBucketCount / EventPlace"""
    rng = np.random.default_rng(6000 + seed)
    nb = len(BUCKET_PLAN)
    ref = random_seq(rng, nb * BLOCK + 300)
    edges = []

    def query():
        q = bytearray(b"N" * len(ref))
        for blk, want in enumerate(BUCKET_PLAN):
            gap = 9 if want > 14 else max(10, BLOCK // max(want, 1) - 1)
            starts = [blk * BLOCK + 12 + i * gap for i in range(want)]
            if want and want <= 14 and blk % 3 == 1:
                starts[-1] = blk * BLOCK + 255                      # the block's last position
            if want and want <= 14 and blk % 3 == 2:
                starts[0] = blk * BLOCK + 1                         # its second
            if want and want <= 14 and blk % 3 == 0:
                starts[0] = blk * BLOCK                             # its first
            for i, s in enumerate(starts):
                L = 8 if want > 14 else 8 + (i & 1)
                q[s:s + L] = ref[s:s + L]
                if s % BLOCK in (255, 0, 1):
                    edges.append(s)
        return bytes(q)

    qs = [query(), query()]
    q3 = bytearray(qs[0]); q3[BLOCK * 6 + 40] = ord("N"); qs.append(bytes(q3))      # (one stretch less in one genome)
    return [ref] + qs, 8, BUCKET_PLAN, sorted(set(edges))


def event_count(O, ref, q, minsize):
    return len(oracles.restatement_events(O, ref, q, minsize)[0]) + len(oracles.restatement_events(O, ref, revcomp(q), minsize)[0])


def trimmed_to(O, ref, p, minsize, target):
    """the query of `p` cut after so many planted stretches (then base by base) that the pair holds exactly `target` events, both
    strands counted with the restatement"""
    ends = [qs + n for _, qs, n, _, _ in p.recs]
    seen = {}

    def count(k):
        if k not in seen:
            seen[k] = event_count(O, ref, p.query[:ends[k - 1]], minsize)
        return seen[k]

    k = min(len(ends), target)
    for _ in range(40):
        c = count(k)
        if c == target:
            return p.query[:ends[k - 1]]
        nk = max(1, min(len(ends), k + (target - c)))
        if nk in seen:
            break
        k = nk
    lo = min(x for x in seen if seen[x] >= target) if any(v >= target for v in seen.values()) else len(ends)
    cut = ends[lo - 1]
    while cut > 0:
        c = event_count(O, ref, p.query[:cut], minsize)
        if c == target:
            return p.query[:cut]
        if c < target:
            break
        cut -= 1
    raise AssertionError("no prefix of the designed query holds exactly %d events" % target)


SCAN_COUNTS = ((512, 1024, 1537, 511), (511, 513, 1024, 1537, 512))


def scan_set(O, counts, seed=0):
    """(seqs, minsize, counts): query g holds exactly counts[g] events (both strands), so that with 512 events per wavefront of the
    scan a pair ends on a wavefront's last lane, the next pair's head is lane 0 of the next, and a pair spans more than three"""
    minsize = 12
    rng = np.random.default_rng(7000 + seed)
    most = max(counts)
    ls = [int(x) for x in rng.integers(12, 17, most + 40)]
    ref = random_seq(rng, needed(ls) + 40)
    qs = []
    for g, c in enumerate(counts):
        kinds = (("sub",), ("sub", "n"), ("sub", "ins", "del"), ("n", "sub", "sub"), ("sub", "del"))[g % 5]
        p = planted(ref, ls, kinds, cycle=False)
        qs.append(trimmed_to(O, ref, p, minsize, c))
    return [ref] + qs, minsize, counts


def tie_set(seed=0):
    """(seqs, minsize): queries that hold one reference stretch twice -- two events with the same l and the same reach, which
    win_join has to order by j -- beside ordinary matches"""
    minsize = 10
    rng = np.random.default_rng(8000 + seed)
    ref = random_seq(rng, 1500)
    p = planted(ref, [25, 40, 18, 60, 33], ("sub", "n", "ins"))
    S = ref[400:430]
    qs = [p.query[:600] + b"N" + S + b"N" + p.query[600:] + b"N" + S,
          S + b"N" + p.query + b"N" + S + b"N" + S,
          p.query]
    return [ref] + qs, minsize
