"""Designed inputs for the SMALL-REGION event search -- SmallPairEvents (parsnp_amd/csrc/engine/kernels.h), GroupedPairEvents and
GroupedPairEventsWide (store_kernels.h) and the bit-plane machinery under them (planes64, W64, W128, pair_diagonals) -- shared by
tests/test_small_pairs.py (the kernel emulation) and tests/test_gpu_small_pairs.py (the device).  Pure Python and numpy; seeded.

The constants below restate the sources; test_generator_matches_the_source reads them out of the sources and compares.

pair_cases      one (reference, query) pair per entry: a stretch of a designed length planted into two UNRELATED random strings, in
                one of the four corners (reference start or end against query start or end) or centred across bit 63 / 64 of the
                128-bit words, bounded by a mismatch on both sides where there is room, with the minimum lengths to search it at.
special_pairs   the other single-pair cases: two stretches on one diagonal around bit 63 / 64, the two outermost diagonals, a side
                shorter than L, m == L and nR == L, N inside a stretch, a stretch held twice by the reference (len == rep' and
                rep' + 1), homopolymers, a 7-base tandem.
ends_batch      5 query genomes of 128, 129, 191, 200 and 257 bases (two stored reverse-complemented, the last one among them),
                windows of 1 .. 128 bases at both genome ends and in the middle.
fields_batch    regions whose packed words of the grouped forms hold the extreme values: e1 = 128, spb = -127 / +127, a
                homopolymer (len 128 over rep' 127).
lanes_batch     70 or 130 query genomes (2 or 3 genomes a lane in step 1 of the grouped forms); per region ONE deciding genome.
tandem_batch    a low-complexity batch built like test_emu_engine.small_region_batch(low_complexity=True), with shorter reference windows.

`python smallgen.py first LIB` runs the smallest batch in a process of its own (the GPU file's first test, under a time limit)."""
import sys
from collections import namedtuple

import numpy as np

SMALL = 128          # small_pair: nR <= 128 && m <= 128 (kernels.h, twice; engine_core.h)
WORD = 64            # W64 where nR <= 64 && m <= 64, W128 otherwise (SmallPairEvents and both grouped forms)
GRP_EVENTS, GRP_PIECES = 8, 32        # kGrpEvents (PM_GRP_EVENTS), kGrpPieces
WIDE_EVENTS, WIDE_PIECES = 32, 128    # kWideEvents, kWidePieces
KMAX = 16            # rep' is measured along K-mer chains, K = min(L, 16): the comparisons zero rep' below K

LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128)
OVER = ((128, 129), (129, 128), (129, 129))       # the first pairs that are not small
STRETCHES = (1, 2, 31, 32, 33, 63, 64, 65, 127)
FIXED_L = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)      # the doubling filter at every k, with and without the rest step
PLACES = ("ss", "se", "es", "ee", "mid")

Pair = namedtuple("Pair", "name ref query planted Ls")          # planted: [(l, j, n)]
Batch = namedtuple("Batch", "name seqs starts lens mins info")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes((c if c in b"ACGT" else ord("N")) for c in s).translate(_COMP)[::-1]


def random_seq(rng, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def other(c, k=0):
    """the (k + 1)-th base that is not c"""
    return [x for x in b"ACGT" if x != c][k % 3]


def occurrences(s, sub):
    n, at = 0, s.find(sub)
    while at >= 0:
        n += 1; at = s.find(sub, at + 1)
    return n


def plant(rng, nR, m, spots):
    """two unrelated random strings; the query carries the reference's bases [l, l + n) at j for every (l, j, n) of spots, and a
    base that differs from the reference's before and behind each stretch where both sides have room (and no other stretch lies)"""
    ref = bytearray(random_seq(rng, nR)); q = bytearray(random_seq(rng, m))
    held = set()
    for l, j, n in spots:
        assert 0 <= l and l + n <= nR and 0 <= j and j + n <= m, (nR, m, spots)
        q[j:j + n] = ref[l:l + n]; held.update(range(j, j + n))
    for l, j, n in spots:
        if l > 0 and j > 0 and j - 1 not in held:
            q[j - 1] = other(ref[l - 1], int(rng.integers(0, 3)))
        if l + n < nR and j + n < m and j + n not in held:
            q[j + n] = other(ref[l + n], int(rng.integers(0, 3)))
    return bytes(ref), bytes(q)


def place(nR, m, n, where):
    """(l, j) of a stretch of n bases: a corner, or centred across bit 63 / 64 (the middle of a shorter side)"""
    mid = lambda side: max(0, min(side - n, WORD - n // 2)) if side > WORD else (side - n) // 2
    return {"ss": (0, 0), "se": (0, m - n), "es": (nR - n, 0), "ee": (nR - n, m - n), "mid": (mid(nR), mid(m))}[where]


def pair_cases(nR, m, thin=False):
    """the designed pairs of one pair of lengths: every stretch length that fits (STRETCHES, the shorter side's whole length and that
    minus 1) at every distinct place, each with L = len - 1, len, len + 1 and two values of FIXED_L that rotate from case to case,
    all kept within 1 .. the shorter side.  thin: four (case, L) combinations a pair, spread over places and kinds of L with an
    offset that moves from pair to pair, and the whole shorter side at L == its length (m == L or nR == L)"""
    short = min(nR, m)
    seed = 1000003 * nR + 1009 * m
    out = []
    i = 0
    for n in sorted({x for x in STRETCHES + (short, short - 1) if 1 <= x <= short}):
        seen = set()
        for where in PLACES:
            l, j = place(nR, m, n, where)
            if (l, j) in seen:
                continue
            seen.add((l, j))
            rng = np.random.default_rng(seed + 31 * i)
            for _ in range(20):       # (a stretch of 8 bases or more is unique in the reference: drawn again if chance repeats it)
                ref, q = plant(rng, nR, m, [(l, j, n)])
                if n < 8 or occurrences(ref, ref[l:l + n]) == 1:
                    break
            Ls = {n - 1, n, n + 1, FIXED_L[i % len(FIXED_L)], FIXED_L[(7 * i + 3) % len(FIXED_L)]}
            out.append(Pair("%dx%d/%d@%s" % (nR, m, n, where), ref, q, [(l, j, n)], tuple(sorted(x for x in Ls if 1 <= x <= short))))
            i += 1
    if not thin:
        return out
    flat = [(p, L) for p in out for L in p.Ls]
    off = (LENGTHS + (129,)).index(nR) * 5 + (LENGTHS + (129,)).index(m) * 3
    pick = {(off + k * len(flat) // 4) % len(flat) for k in range(4)}
    pick |= {x for x, (p, L) in enumerate(flat) if p.planted[0] == (0, 0, short) and L == short}
    by = {}
    for x in sorted(pick):
        by.setdefault(flat[x][0].name, (flat[x][0], []))[1].append(flat[x][1])
    return [p._replace(Ls=tuple(Ls)) for p, Ls in by.values()]


def special_pairs():
    """{name: Pair}: the single-pair cases that are no corner stretch (the tests assert what each is for from the restatement)"""
    out = {}
    rng = np.random.default_rng(4242)
    # two stretches on one diagonal, one mismatch between them on bit 63 and on bit 64 of the difference word (bit t is the query
    # position where d >= 0 and the reference position where d < 0)
    for gap in (63, 64):
        for d in (0, 5, -5):
            lo, hi = 20, 110
            a = (lo + max(d, 0), lo + max(-d, 0), gap - lo)
            b = (gap + 1 + max(d, 0), gap + 1 + max(-d, 0), hi - gap - 1)
            ref, q = plant(rng, 128, 128, [a, b])
            out["split%d/d%+d" % (gap, d)] = Pair("split%d/d%+d" % (gap, d), ref, q, [a, b], (1, gap - lo, gap - lo + 1, hi - gap - 1, hi - gap))
    # the two outermost diagonals of one pair: d = -(m - L) (reference start against query end) and d = nR - L
    for nR, m, L in ((128, 128, 12), (65, 128, 9), (64, 64, 10), (128, 33, 17), (127, 96, 32)):
        ref, q = plant(rng, nR, m, [(0, m - L, L), (nR - L, 0, L)])
        out["outer%dx%d" % (nR, m)] = Pair("outer%dx%d" % (nR, m), ref, q, [(0, m - L, L), (nR - L, 0, L)], (L - 1, L, L + 1))
    # a side shorter than L (no event, no read of a negative diagonal range), m == L and nR == L
    for nR, m, L in ((10, 50, 11), (50, 10, 11), (128, 5, 6), (64, 65, 65), (1, 128, 2)):
        n = min(nR, m)
        ref, q = plant(rng, nR, m, [(0, 0, n)])
        out["shorter%dx%d" % (nR, m)] = Pair("shorter%dx%d" % (nR, m), ref, q, [(0, 0, n)], (L, L + 1, 128))
    for nR, m in ((128, 40), (40, 128), (65, 65), (128, 128), (64, 17), (17, 64)):
        n = min(nR, m)
        l, j = (nR - n) // 2, (m - n) // 2
        ref, q = plant(rng, nR, m, [(l, j, n)])
        out["whole%dx%d" % (nR, m)] = Pair("whole%dx%d" % (nR, m), ref, q, [(l, j, n)], (n,))
    # N: inside the stretch on one side, then on both sides at the same place; an N run that reaches the end of a side
    ref, q = plant(rng, 128, 128, [(40, 44, 60)])
    rn, qn = bytearray(ref), bytearray(q)
    rn[70] = qn[74] = ord("N")
    out["n/reference"] = Pair("n/reference", bytes(rn), q, [(40, 44, 30), (71, 75, 29)], (4, 29, 30, 31))
    out["n/query"] = Pair("n/query", ref, bytes(qn), [(40, 44, 30), (71, 75, 29)], (4, 29, 30, 31))
    out["n/both"] = Pair("n/both", bytes(rn), bytes(qn), [(40, 44, 60)], (4, 59, 60, 61))
    ref, q = plant(rng, 128, 100, [(98, 70, 30)])
    out["n/run_to_end"] = Pair("n/run_to_end", ref[:118] + b"N" * 10, q[:90] + b"N" * 10, [(98, 70, 30)], (1, 10, 11, 29, 30))
    out["n/run_one_side"] = Pair("n/run_one_side", ref[:118] + b"N" * 10, q, [(98, 70, 20)], (1, 10, 20, 21))
    # uniqueness in R: a reference of 128 bases holds a stretch of 20 twice; the query holds the stretch alone (len == rep': no
    # event) and the stretch with the base that follows its first copy (len == rep' + 1: an event)
    ref = bytearray(random_seq(rng, 128))
    ref[70:90] = ref[5:25]
    ref[90] = other(ref[25]); ref[69] = other(ref[4])
    q = bytearray(random_seq(rng, 100))
    q[10:30] = ref[5:25]; q[9] = other(ref[4], 1) if other(ref[4], 1) != ref[69] else other(ref[4], 2)
    q[30] = [x for x in b"ACGT" if x not in (ref[25], ref[90])][0]
    q[50:71] = ref[5:26]; q[49] = other(ref[4], 1) if other(ref[4], 1) != ref[69] else other(ref[4], 2)
    q[71] = other(ref[26])
    out["repeat"] = Pair("repeat", bytes(ref), bytes(q), [(5, 10, 20), (5, 50, 21)], (10, 16, 17, 20, 21, 22))
    # homopolymers: 128 x A against itself (len 128 over rep' 127), against 127 x A + C
    out["homopolymer"] = Pair("homopolymer", b"A" * 128, b"A" * 128, [(0, 0, 128)], (1, 2, 16, 17, 64, 127, 128))
    out["homopolymer/c"] = Pair("homopolymer/c", b"A" * 128, b"A" * 127 + b"C", [(1, 0, 127)], (1, 2, 16, 17, 64, 127, 128))
    out["homopolymer/c_ref"] = Pair("homopolymer/c_ref", b"A" * 127 + b"C", b"A" * 128, [(0, 1, 127)], (1, 16, 127, 128))
    # many events in one pair: a 7-base tandem of 128 against tandem pieces (the first event of a lane goes through
    # wave_reserve01, the others through the slice's atomic)
    unit = b"ACGTTGA"
    tandem = (unit * 19)[:128]
    piece = bytearray((unit * 19)[3:103]); piece[40] = other(piece[40]); piece[77] = other(piece[77])
    long_piece = bytearray((unit * 19)[2:130]); long_piece[50] = other(long_piece[50]); long_piece[99] = other(long_piece[99])
    out["tandem"] = Pair("tandem", tandem[:33], bytes(long_piece), [], (2, 3, 4, 7, 8, 15))      # (unique in R: the stretches that reach the window's end)
    out["tandem/short_ref"] = Pair("tandem/short_ref", tandem[:22], bytes(piece), [], (2, 3, 4))
    out["tandem/whole"] = Pair("tandem/whole", tandem, bytes(piece), [], (2, 8))                 # (no stretch of 100 bases is unique in 128 of tandem)
    return out


# ------------------------------------------------------------------------------------------ batches
def _flip(glen, start, ln, stored_reverse):
    return glen - start - ln if stored_reverse else start


QLENS = (128, 129, 191, 200, 257)
REVERSED = (2, 5)          # (1-based) stored reverse-complemented; the last genome is one of them
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)


def ends_batch(seed=77):
    """the reference is H (128 bases) + 7 + T (128); a query genome of n bases is its own copy of H and the last n - 128 bases of
    (7 + T), with two or three private substitutions.  Regions: a window of every width of WIDTHS at the start, at the END of every
    genome (its own end: the windows of one region lie at different places of T) and in the middle, each at two or three minimum
    lengths of FIXED_L; and regions in which a genome's piece has length 0, 1 and L - 1 beside full pieces.  Windows of a genome that
    is stored reverse-complemented are requested where the reverse complement put them: qs + m == glen at the start, qs == 0 at the end"""
    rng = np.random.default_rng(seed)
    H, F, T = random_seq(rng, 128), random_seq(rng, 7), random_seq(rng, 128)
    ref = H + F + T
    fwd = [ref]
    for g, n in enumerate(QLENS, 1):
        s = bytearray(H + (F + T)[len(F + T) - (n - 128):] if n > 128 else H)
        for at in (10 + 17 * g, 70 + 9 * g, n - 5 - 11 * g):
            s[at] = other(s[at], g)
        fwd.append(bytes(s))
    seqs = [fwd[0]] + [revcomp(s) if g in REVERSED else s for g, s in enumerate(fwd[1:], 1)]
    rows = []       # (what, width, L, [(start, len) in forward coordinates per genome])
    i = 0
    for w in WIDTHS:
        cands = [L for L in FIXED_L if L <= w]
        for what in ("start", "end", "middle", "middle2"):
            Ls = sorted({cands[i % len(cands)], cands[(3 * i + 1) % len(cands)], cands[-1 - (i % 2)] if len(cands) > 1 else cands[0]})
            for L in Ls:
                s0 = (5 * i + 3) % 32 + (24 if what == "middle2" else 0)
                wins = []
                for g, s in enumerate(fwd):
                    n = len(s)
                    st = 0 if what == "start" else n - w if what == "end" else min(s0, n - w)
                    wins.append((st, w))
                rows.append((what, w, L, wins))
                i += 1
    for L in (8, 16, 33):          # a genome's piece of length 0, 1 and L - 1 beside full pieces
        wins = [(20, 64)] * len(fwd)
        wins[1] = (20, 0); wins[3] = (20, 1); wins[4] = (20, L - 1); wins[5] = (20 + 64 - (L - 1), L - 1)
        rows.append(("short", 64, L, wins))
    return _batch("ends", seqs, fwd, rows, REVERSED)


def _batch(name, seqs, fwd, rows, reversed_):
    nreg, ngen = len(rows), len(seqs)
    starts = np.zeros((nreg, ngen), np.int64); lens = np.zeros_like(starts); mins = np.zeros(nreg, np.int32)
    for r, (what, w, L, wins) in enumerate(rows):
        mins[r] = L
        for g, (st, ln) in enumerate(wins):
            starts[r, g] = _flip(len(fwd[g]), st, ln, g in reversed_); lens[r, g] = ln
    return Batch(name, seqs, starts, lens, mins, dict(rows=rows, reversed=tuple(reversed_)))


def fields_batch(seed=91):
    """4 query genomes (genome 2 stored reverse-complemented); every genome is private spacers around the same designed segments:
      whole    128 bases, the same in every genome: the multi-MUM is the whole window (e1 = 128, len = 128)
      minus    reference: 127 bases of A, C, G and ONE T at position 127; queries: T + 127 x N -- the only event is
               (l, j, len) = (127, 0, 1) at L = 1, the T is unique in the window (spb = j - l = -127)
      plus     reference: T + 127 bases of A, C, G; queries: 127 x N + T (spb = +127)
      poly     128 x A in every genome (len 128 over rep' 127)
    and every region is requested at two minimum lengths."""
    rng = np.random.default_rng(seed)
    acg = lambda n: random_seq(rng, n, b"ACG")
    segs = [("whole", random_seq(rng, 128), None), ("minus", acg(127) + b"T", b"T" + b"N" * 127), ("plus", b"T" + acg(127), b"N" * 127 + b"T"),
            ("poly", b"A" * 128, None)]
    nq, rev = 4, (2,)
    fwd, at = [], {}
    for g in range(nq + 1):
        s = b""
        for name, r, q in segs:
            s += random_seq(rng, 13 + 3 * g + len(at) % 5)
            at[(name, g)] = len(s)
            s += r if g == 0 or q is None else q
        fwd.append(s + random_seq(rng, 11 + g))
    seqs = [fwd[0]] + [revcomp(s) if g in rev else s for g, s in enumerate(fwd[1:], 1)]
    rows = []
    for name, Ls in (("whole", (128, 20)), ("minus", (1, 1)), ("plus", (1, 1)), ("poly", (16, 128, 1))):
        for L in Ls:
            rows.append((name, 128, L, [(at[(name, g)], 128) for g in range(nq + 1)]))
    return _batch("fields", seqs, fwd, rows, rev)


def deciders(nq):
    return [d for d in (1, 63, 64, 65, 128) if d < nq] + [nq]


def lanes_batch(nq, seed=5):
    """nq = 70 / 130 query genomes: (nq + 63) / 64 = 2 / 3 genomes a lane in step 1 of the grouped forms.  Per deciding genome d
    (index 1, 63, 64, 65, 128, last) two regions of 90 bases that every genome holds in one of three versions: in the first, d's
    piece is the only SHORT one (40 bases); in the second, d alone has a substitution in the middle of the window.  One more region
    is 128 x A in the reference and in most genomes, with C at position 128 - g in genome g = 1 .. 40: more than kGrpPieces distinct
    pieces, so the wide form takes it where it runs (len 128 over rep' 127 in the wide form's packed word), and a multi-MUM of
    the window's last 88 bases that begins at another query position in each of the 40.  Genomes with
    g % 7 == 3, and genome 64, are stored reverse-complemented."""
    rng = np.random.default_rng(seed + nq)
    ds = deciders(nq)
    nreg = 2 * len(ds)
    base = bytearray(random_seq(rng, 100 * nreg + 20))
    poly_at = len(base)
    base += b"A" * 128 + random_seq(rng, 9)
    rev = tuple(g for g in range(1, nq + 1) if g % 7 == 3 or g == 64)
    fwd = [bytes(base)]
    for g in range(1, nq + 1):
        s = bytearray(base)
        v = g % 3
        for r in range(nreg):
            if v:
                s[100 * r + 10 + 5 + 3 * v] = other(s[100 * r + 10 + 5 + 3 * v], v)
        if g <= 40:
            s[poly_at + 128 - g] = ord("C")
        fwd.append(s)
    rows = []
    for x, d in enumerate(ds):
        for kind in (0, 1):
            r = 2 * x + kind
            wins = [(100 * r + 10, 90)] * (nq + 1)
            if kind == 0:
                wins[d] = (100 * r + 10 + 25, 40)
            else:
                fwd[d][100 * r + 10 + 45] = other(fwd[d][100 * r + 10 + 45], 2)
            rows.append(("short" if kind == 0 else "sub", 90, (12, 9, 16, 11, 20, 8)[x % 6], wins))
    rows.append(("poly", 128, 3, [(poly_at, 128)] * (nq + 1)))
    fwd = [bytes(s) for s in fwd]
    seqs = [fwd[0]] + [revcomp(s) if g in rev else s for g, s in enumerate(fwd[1:], 1)]
    b = _batch("lanes%d" % nq, seqs, fwd, rows, rev)
    b.info["deciders"] = ds
    return b


def tandem_batch(seed=41, nq=24, n_regions=48, distinct=3, ref_len=(24, 34), q_len=(40, 70), minsize=(2, 5)):
    """a low-complexity batch as test_emu_engine.small_region_batch(low_complexity=True) builds it -- a 7-base tandem of 4 kb, the
    query genomes one of `distinct` versions with 3 % substitutions, every fifth genome with an inverted stretch, windows with
    some jitter in their lengths -- but with the reference's window (24 .. 33 bases) shorter than the queries' (40 .. 69) and minimum
    lengths of 2 .. 4: windows of equal lengths hold less than one event a pair (a stretch of a tandem is unique in the reference
    window only where it reaches the window's end), these hold five to ten.  Ten bases of their own at the head of every window,
    the same in every genome, give the region a multi-MUM."""
    rng = np.random.default_rng(seed)
    glen = 4000
    ref = (random_seq(rng, 7) * (glen // 7 + 1))[:glen]

    def mutate(s):
        a = np.frombuffer(s, np.uint8).copy()
        hit = rng.random(len(a)) < 0.03
        a[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        return a.tobytes()

    versions = [ref] + [mutate(ref) for _ in range(distinct - 1)]
    seqs = [ref]
    for g in range(nq):
        q = versions[int(rng.integers(0, distinct))]
        if g % 5 == 4:
            a = glen // 4; b = a + glen // 3
            q = q[:a] + revcomp(q[a:b]) + q[b:]
        seqs.append(q)
    seqs = [bytearray(s) for s in seqs]
    starts = np.zeros((n_regions, nq + 1), np.int64); lens = np.zeros_like(starts); mins = np.zeros(n_regions, np.int32)
    for r in range(n_regions):
        ln = int(rng.integers(*q_len)); st = int(rng.integers(0, glen - 140))
        for g in range(nq + 1):
            jitter = int(rng.integers(-3, 4)) if rng.random() < 0.2 else 0
            lens[r, g] = max(0, min(128, ln + jitter)); starts[r, g] = st
        lens[r, 0] = int(rng.integers(*ref_len))
        mins[r] = int(rng.integers(*minsize))
        word = random_seq(rng, 10)
        for s in seqs:
            s[st:st + 10] = word
    return Batch("tandem", [bytes(s) for s in seqs], starts, lens, mins, dict(rows=None, reversed=()))


def pieces(b, r):
    """the strings of region r, the reference's first, as the engine reads them from the stored genomes"""
    return [b.seqs[g][b.starts[r, g]:b.starts[r, g] + b.lens[r, g]] for g in range(len(b.seqs))]


def window_alignments(b):
    """{p & 31} over every window of the batch, as planes64 meets them: the forward strand's start and the reverse strand's
    (glen - qs - m); the strands begin on a block boundary"""
    out = set()
    for r in range(b.starts.shape[0]):
        for g in range(len(b.seqs)):
            qs, m = int(b.starts[r, g]), int(b.lens[r, g])
            out.add(qs & 31)
            if g:
                out.add((len(b.seqs[g]) - qs - m) & 31)
    return out


ROUTES = (("pairwise", {"group_small": 0}), ("grouped", {"group_small": 1, "group_wide": 0}), ("wide", {"group_small": 1, "group_wide": 1}))


def run_routes(lib, b, routes=ROUTES):
    """{route: (the regions' multi-MUMs, the counts of pm_last_timing)}, one session per route"""
    from parsnp_amd.binding import Session
    out = {}
    for route, tunes in routes:
        with Session(lib, b.seqs) as s:
            for k, v in tunes.items():
                s.tune(k, v)
            got = s.multi_mum_batch(b.starts, b.lens, b.mins)
            out[route] = (got, {k: v for k, v in s.last_timing()})
    return out


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "first":
    from parsnp_amd.binding import Lib
    import oracles
    lib = Lib(sys.argv[2]); O = oracles.load_restatement()
    b = fields_batch()
    runs = run_routes(lib, b)
    for r in range(b.starts.shape[0]):
        want = oracles.restatement_multi_mum(O, pieces(b, r), int(b.mins[r]), 1)
        for route, (got, counts) in runs.items():
            assert all(np.array_equal(x, y) for x, y in zip(want[:4], got[r][:4])), (b.name, r, route)
    print({route: int(c["n_grouped"]) for route, (_, c) in runs.items()}, flush=True)
    print("first ok")
